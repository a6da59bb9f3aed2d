"""uint16 / int16 frames on the device, natively (the typed entries nsof_farneback_px*, include/nsof.h).

A 16-bit pixel converts to float32 exactly, so every check here compares against the float32 path on
``frame.astype(np.float32)``, bit for bit (``array_equal`` of the flow's bits): lone calls, device batches and
sequences, work lists of crops (the scale-8 level of large crops included), the gated ROI sequence, the host list entry
and the pyramid stage.  A route check pins the launches: a 16-bit batch issues the 8-bit batch's prep and expansion
launch counts (the three-level pyramid launch and level 0 formed inside the expansion).  Refusals return NSOF_EINVAL
before anything is launched."""
import numpy as np
import pytest

from nsof.errors import NsofValueError
from test_float_reference import PARAM_SETS, shifted_pair
from test_float_worklists_gpu import ROI_TABLE, _roi_tensors

pytestmark = pytest.mark.gpu

ARGS = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags")
DTYPES = ["uint16", "int16"]


def _args(p):
    return [getattr(p, k) for k in ARGS]


def _same(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.fixture(params=[0, 1], ids=["plain", "fma"])
def pyr_fma(request, ctx):
    from nsof import _lib
    saved = ctx.get_option(_lib.OPT_PYR_FMA)
    ctx.set_option(_lib.OPT_PYR_FMA, request.param)
    yield request.param
    ctx.set_option(_lib.OPT_PYR_FMA, saved)


def _full_range(dtype):
    info = np.iinfo(dtype)
    return float(info.min), float(info.max)


def _pair16(seed, h, w, dtype, content="smooth"):
    """(prev, next) of dtype: a smooth shifted pattern over the type's full range, noise, a 0 / max checkerboard or
    constant frames."""
    dt = np.dtype(dtype)
    lo, hi = _full_range(dt)
    if content == "smooth":
        a, b = shifted_pair(seed, h, w, lo, hi)
        return np.clip(np.rint(a), lo, hi).astype(dt), np.clip(np.rint(b), lo, hi).astype(dt)
    rng = np.random.default_rng(seed)
    if content == "noise":
        return (rng.integers(int(lo), int(hi) + 1, (h, w)).astype(dt), rng.integers(int(lo), int(hi) + 1, (h, w)).astype(dt))
    if content == "checker":
        yy, xx = np.mgrid[0:h, 0:w]
        c = np.where((yy + xx) % 2 == 0, lo if dt.kind == "i" else 0, hi).astype(dt)
        return c, np.roll(c, 1, axis=1)
    return np.full((h, w), hi, dt), np.full((h, w), lo, dt)   # constant


def _up(arr, dev):
    """A host array on the device (tensors are made on the host and copied: uint16 tensors need no device kernels)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def _f32_flow(nsof_lib, ctx, a, b, p, **kw):
    return nsof_lib.calcOpticalFlowFarneback(a.astype(np.float32), b.astype(np.float32), None, *_args(p), ctx=ctx, **kw)


# ---- 1. lone calls through nsof_farneback_px ----------------------------------------------------------------------
LONE_SHAPES = [(96, 256), (72, 200), (61, 191), (45, 385), (17, 23), (9, 12)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lone_calls_equal_f32(nsof_lib, ctx, pyr_fma, exact, name, dtype):
    p = PARAM_SETS[name]
    for i, (h, w) in enumerate(LONE_SHAPES):
        a, b = _pair16(3 + i, h, w, dtype)
        got = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx, exact=exact)
        assert _same(got, _f32_flow(nsof_lib, ctx, a, b, p, exact=exact)), (h, w)


@pytest.mark.parametrize("content", ["noise", "checker", "constant"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_lone_calls_extreme_content(nsof_lib, ctx, pyr_fma, dtype, content):
    for name in ("A", "B"):
        p = PARAM_SETS[name]
        for (h, w) in ((64, 192), (31, 45)):
            a, b = _pair16(9, h, w, dtype, content)
            got = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx)
            assert _same(got, _f32_flow(nsof_lib, ctx, a, b, p)), (name, h, w)


@pytest.mark.parametrize("dtype", DTYPES)
def test_lone_call_1080p(nsof_lib, ctx, pyr_fma, dtype):
    p = PARAM_SETS["A"]
    a, b = _pair16(21, 1080, 1920, dtype)
    got = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx)
    assert _same(got, _f32_flow(nsof_lib, ctx, a, b, p))
    # a column-strided view is made contiguous, as the 8-bit route does
    wide = np.zeros((1080, 3840), a.dtype)
    wide[:, ::2] = a
    assert _same(nsof_lib.calcOpticalFlowFarneback(wide[:, ::2], b, None, *_args(p), ctx=ctx), got)


# ---- 2. farneback_batch / farneback_sequence ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_batch_and_sequence(nsof_lib, ctx, torch_dev, pyr_fma, name, dtype):
    import torch
    from nsof.farneback import farneback_batch, farneback_sequence
    p = PARAM_SETS[name]
    h, w = 96, 256
    for n in (1, 2, 24):   # 1 / 2 pairs: the small-batch form (exact_lat); 24 pairs x 2 strips: the uniform driver
        frames = np.stack([_pair16(30 + k // 2, h, w, dtype)[k % 2] for k in range(n + 1)])
        tf = _up(frames, torch_dev)
        ff = _up(frames.astype(np.float32), torch_dev)
        want = torch.empty((n, h, w, 2), dtype=torch.float32, device=torch_dev)
        farneback_batch(ff[:n], ff[1:], want, n, h, w, p, ctx=ctx)
        got = torch.empty_like(want)
        farneback_batch(tf[:n].contiguous(), tf[1:].contiguous(), got, n, h, w, p, ctx=ctx)
        raw = torch.empty_like(want)
        a16, b16 = tf[:n].contiguous(), tf[1:].contiguous()
        farneback_batch(a16.data_ptr(), b16.data_ptr(), raw, n, h, w, p, dtype=getattr(np, dtype), ctx=ctx)
        seq = torch.empty_like(want)
        farneback_sequence(tf, seq, n + 1, h, w, p, ctx=ctx)
        # padded rows, and frames that start at an odd element (2-byte aligned only: the scalar level 0)
        hpad = np.zeros((n + 1, h, w + 3), frames.dtype)
        hpad[:, :, 1:w + 1] = frames
        pad = _up(hpad, torch_dev)
        view = pad[:, :, 1:w + 1]
        assert view.data_ptr() % 4 == 2
        padded = torch.empty_like(want)
        farneback_sequence(view, padded, n + 1, h, w, p, row_stride=(w + 3) * 2, frame_stride=h * (w + 3) * 2, ctx=ctx)
        ctx.synchronize()
        for t in (got, raw, seq, padded):
            assert _same(t.cpu().numpy(), want.cpu().numpy()), n


# ---- 3. device work lists -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_device_pairs_on_crops(nsof_lib, ctx, torch_dev, pyr_fma, name, dtype):
    import torch
    from nsof.farneback import farneback_pairs_16_dev, farneback_pairs_f32_dev
    p = PARAM_SETS[name]
    H, W = 120, 404   # noqa: N806
    a, b = _pair16(11, H, W, dtype)
    ta, tb = _up(a, torch_dev), _up(b, torch_dev)
    fa, fb = _up(a.astype(np.float32), torch_dev), _up(b.astype(np.float32), torch_dev)
    # aligned starts (vector level 0), odd starts and widths, strip edges
    crops = [(0, H, 0, W), (8, 72, 4, 200), (5, 60, 16, 216), (10, 70, 3, 196), (0, 9, 1, 13), (20, 81, 37, 102),
             (1, 120, 11, 396)]
    canvas = torch.zeros((len(crops), H, W, 2), dtype=torch.float32, device=torch_dev)
    farneback_pairs_16_dev([(ta[y0:y1, x0:x1], tb[y0:y1, x0:x1]) for (y0, y1, x0, x1) in crops],
                           [canvas[i, y0:y1, x0:x1] for i, (y0, y1, x0, x1) in enumerate(crops)], p, ctx=ctx)
    ref = torch.zeros_like(canvas)
    farneback_pairs_f32_dev([(fa[y0:y1, x0:x1], fb[y0:y1, x0:x1]) for (y0, y1, x0, x1) in crops],
                            [ref[i, y0:y1, x0:x1] for i, (y0, y1, x0, x1) in enumerate(crops)], p, ctx=ctx)
    ctx.synchronize()
    host, want = canvas.cpu().numpy(), ref.cpu().numpy()
    for i, (y0, y1, x0, x1) in enumerate(crops):
        assert _same(host[i, y0:y1, x0:x1], want[i, y0:y1, x0:x1]), (y0, y1, x0, x1)
        host[i, y0:y1, x0:x1] = 0
        assert not host[i].any(), "written outside the crop"


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_pairs_beyond_job_tables(nsof_lib, ctx, torch_dev, dtype):
    """40 crops of 200 columns: more strip jobs than the small-batch form takes (k_iterate_x's job tables)."""
    import torch
    from nsof.farneback import farneback_pairs_16_dev, farneback_pairs_f32_dev
    p = PARAM_SETS["A"]
    a, b = _pair16(17, 128, 420, dtype)
    ta, tb = _up(a, torch_dev), _up(b, torch_dev)
    crops = [(y, y + 40 + y % 7, x, x + 200) for y in range(0, 80, 10) for x in (0, 1, 50, 103, 204)]
    assert sum((x1 - x0 + 191) // 192 for (_, _, x0, x1) in crops) > 64
    out = [torch.empty((y1 - y0, x1 - x0, 2), dtype=torch.float32, device=torch_dev) for (y0, y1, x0, x1) in crops]
    ref = [torch.empty_like(o) for o in out]
    farneback_pairs_16_dev([(ta[y0:y1, x0:x1], tb[y0:y1, x0:x1]) for (y0, y1, x0, x1) in crops], out, p, ctx=ctx)
    fa, fb = _up(a.astype(np.float32), torch_dev), _up(b.astype(np.float32), torch_dev)
    farneback_pairs_f32_dev([(fa[y0:y1, x0:x1], fb[y0:y1, x0:x1]) for (y0, y1, x0, x1) in crops], ref, p, ctx=ctx)
    ctx.synchronize()
    for o, r in zip(out, ref):
        assert _same(o.cpu().numpy(), r.cpu().numpy())


@pytest.mark.parametrize("dtype", DTYPES)
def test_device_pairs_scale8_level(nsof_lib, ctx, torch_dev, pyr_fma, dtype):
    """8 crops of 1600 x 900 (set A: a scale-8 level with 19 taps, the tiled kernel's largest footprint)."""
    import torch
    from nsof.farneback import farneback_pairs_16_dev, farneback_pairs_f32_dev
    p = PARAM_SETS["A"]
    a, b = _pair16(23, 1000, 1700, dtype)
    ta, tb = _up(a, torch_dev), _up(b, torch_dev)
    fa, fb = _up(a.astype(np.float32), torch_dev), _up(b.astype(np.float32), torch_dev)
    crops = [(k * 13, k * 13 + 900, k * 11 + (k & 1), k * 11 + (k & 1) + 1600) for k in range(8)]
    out = torch.empty((8, 900, 1600, 2), dtype=torch.float32, device=torch_dev)
    ref = torch.empty_like(out)
    farneback_pairs_16_dev([(ta[y0:y1, x0:x1], tb[y0:y1, x0:x1]) for (y0, y1, x0, x1) in crops], list(out), p, ctx=ctx)
    farneback_pairs_f32_dev([(fa[y0:y1, x0:x1], fb[y0:y1, x0:x1]) for (y0, y1, x0, x1) in crops], list(ref), p, ctx=ctx)
    ctx.synchronize()
    assert _same(out.cpu().numpy(), ref.cpu().numpy())


# ---- 4. gated ROI sequence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate_frame", [0, 1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_roi_sequence_16(nsof_lib, ctx, torch_dev, dtype, name, gate_frame):
    import torch
    from nsof.farneback import farneback_roi_sequence_16_dev, farneback_roi_sequence_f32_dev
    p = PARAM_SETS[name]
    H, W = 120, 404   # noqa: N806  (the rectangles of ROI_TABLE, overlapping crops included)
    counts, rects = _roi_tensors(torch_dev)
    n = len(ROI_TABLE)
    fr = np.stack([_pair16(50 + k // 2, H, W, dtype)[k % 2] for k in range(n)])
    t16 = _up(fr, torch_dev)
    g16 = torch.empty((n - 1, H, W, 2), dtype=torch.float32, device=torch_dev)
    c16 = farneback_roi_sequence_16_dev(t16, counts, rects, g16, p, gate_frame=gate_frame, ctx=ctx)
    g32 = torch.empty_like(g16)
    c32 = farneback_roi_sequence_f32_dev(_up(fr.astype(np.float32), torch_dev), counts, rects, g32, p, gate_frame=gate_frame, ctx=ctx)
    ctx.synchronize()
    assert c16 == c32 and c16[0] >= 3
    assert _same(g16.cpu().numpy(), g32.cpu().numpy())


# ---- 5. host list entry -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_list_entry(nsof_lib, ctx, pyr_fma, dtype):
    from nsof import _lib
    from nsof.farneback import pinned_empty
    p = PARAM_SETS["B"]
    a, b = _pair16(5, 120, 404, dtype)
    pa, pb = pinned_empty(a.shape, a.dtype), pinned_empty(b.shape, b.dtype)
    pa[...], pb[...] = a, b
    pairs = [(a, b), (a[3:90, 7:250], b[3:90, 7:250]), (pa, pb), (pa[1:40, 1:41], pb[1:40, 1:41]), (a[:17, :23], b[:17, :23])]
    flows = [np.zeros((q.shape[0], q.shape[1], 2), np.float32) for q, _ in pairs]
    descs = (_lib.PairDesc * len(pairs))()
    for d, (q, r), f in zip(descs, pairs, flows):
        d.prev, d.prev_stride, d.next, d.next_stride = q.ctypes.data, q.strides[0], r.ctypes.data, r.strides[0]
        d.width, d.height, d.flow, d.flow_stride = q.shape[1], q.shape[0], f.ctypes.data, f.strides[0]
    pt = _lib.PIXEL_U16 if dtype == "uint16" else _lib.PIXEL_S16
    ctx.check(ctx._lib.nsof_farneback_px_batch(ctx.ptr, pt, len(descs), descs, *_args(p)), "px_batch")
    for (q, r), f in zip(pairs, flows):
        assert _same(f, _f32_flow(nsof_lib, ctx, q, r, p)), q.shape


# ---- 6. pyramid stage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_stage_pyr_level_px(nsof_lib, ctx, torch_dev, pyr_fma, dtype, name):
    import torch
    from nsof import _lib
    p = PARAM_SETS[name]
    pt = _lib.PIXEL_U16 if dtype == "uint16" else _lib.PIXEL_S16
    a, _ = _pair16(8, 200, 416, dtype)
    t16 = _up(a, torch_dev)
    t32 = _up(a.astype(np.float32), torch_dev)
    for (y0, y1, x0, x1) in ((0, 200, 0, 416), (3, 190, 5, 402)):   # dense, cropped (odd start)
        v16, v32 = t16[y0:y1, x0:x1], t32[y0:y1, x0:x1]
        h, w = y1 - y0, x1 - x0
        for k in range(nsof_lib.effective_levels(w, h, p.pyr_scale, p.levels) + 1):
            wk, hk = nsof_lib.level_size(w, h, p.pyr_scale, k)[:2]
            o16 = torch.full((hk, wk), -1.0, dtype=torch.float32, device=torch_dev)
            o32 = torch.full_like(o16, -2.0)
            ctx.check(ctx._lib.nsof_stage_pyr_level_px(ctx.ptr, pt, 1, v16.data_ptr(), 416 * 2, 0, w, h, p.pyr_scale, k,
                                                       o16.data_ptr()), "stage px")
            ctx.check(ctx._lib.nsof_stage_pyr_level_f32(ctx.ptr, 1, v32.data_ptr(), 416 * 4, 0, w, h, p.pyr_scale, k,
                                                        o32.data_ptr()), "stage f32")
            ctx.synchronize()
            assert _same(o16.cpu().numpy(), o32.cpu().numpy()), (y0, x0, k)


# ---- 7. routes: the 8-bit path's launches ---------------------------------------------------------------------------
def test_route_launch_counts_match_u8(nsof_lib, ctx, torch_dev, pyr_fma):
    """A 1080p set-A batch of 16-bit frames issues exactly the prep and expansion launches of the same batch in 8 bits:
    the three-level pyramid launch (k_prep_decim3) and level 0 formed inside the expansion (plain variant)."""
    import torch
    from nsof import _lib
    from nsof.farneback import farneback_batch
    p = PARAM_SETS["A"]
    n, h, w = 2, 1080, 1920
    flow = torch.empty((n, h, w, 2), dtype=torch.float32, device=torch_dev)
    counts = {}
    for dtype in ("uint8", "uint16", "int16"):
        fr = _up(np.zeros((2 * n, h, w), dtype), torch_dev)
        ctx.prof_enable(_lib.K_PREP, _lib.K_POLYEXP)
        try:
            farneback_batch(fr[:n], fr[n:], flow, n, h, w, p, ctx=ctx)
            counts[dtype] = (ctx.prof_collect(_lib.K_PREP)[1], ctx.prof_collect(_lib.K_POLYEXP)[1])
        finally:
            ctx.prof_enable()
    assert counts["uint16"] == counts["uint8"] == counts["int16"], counts
    assert counts["uint8"][0] > 0


# ---- 8. U8 / F32 through the typed entries ----------------------------------------------------------------------------
def test_typed_entries_equal_twins(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import _lib, synth
    p = PARAM_SETS["A"]
    a, b = synth.make_pair(4, 72, 200)
    f_tw, f_px = np.zeros((72, 200, 2), np.float32), np.ones((72, 200, 2), np.float32)
    for pt, q, r, twin in ((_lib.PIXEL_U8, a, b, "nsof_farneback_u8"),
                           (_lib.PIXEL_F32, a.astype(np.float32), b.astype(np.float32), "nsof_farneback_f32")):
        host = (q.ctypes.data, q.strides[0], r.ctypes.data, r.strides[0], 200, 72)
        ctx.check(getattr(ctx._lib, twin)(ctx.ptr, *host, f_tw.ctypes.data, 1600, *_args(p)), twin)
        ctx.check(ctx._lib.nsof_farneback_px(ctx.ptr, pt, *host, f_px.ctypes.data, 1600, *_args(p)), "px")
        assert _same(f_px, f_tw), pt
        tq, tr = _up(q, torch_dev), _up(r, torch_dev)
        o_tw, o_px = torch.zeros((1, 72, 200, 2), device=torch_dev), torch.ones((1, 72, 200, 2), device=torch_dev)
        px = q.itemsize
        dev = (tq.data_ptr(), tr.data_ptr(), 200 * px, 72 * 200 * px, 200, 72)
        ctx.check(getattr(ctx._lib, twin + "_batch_dev")(ctx.ptr, 1, *dev, o_tw.data_ptr(), *_args(p)), twin)
        ctx.check(ctx._lib.nsof_farneback_px_batch_dev(ctx.ptr, pt, 1, *dev, o_px.data_ptr(), *_args(p)), "px")
        ctx.synchronize()
        assert _same(o_px.cpu().numpy(), o_tw.cpu().numpy()) and _same(o_px[0].cpu().numpy(), f_tw), pt

        # Every other forwarder against its typed entry, on the same arguments: the same bits.  (The Python layer calls the
        # typed entries only, so this is what runs the nsof_farneback_u8* / nsof_farneback_f32* exports; one that named the
        # wrong pixel type would read the frames at another pixel size, or be refused for their layout.)
        def both(forwarder, typed, args, shape, written=(...,)):
            outs = []
            for entry, lead in ((forwarder, ()), (typed, (pt,))):
                o = torch.full(shape, float(len(outs)), dtype=torch.float32, device=torch_dev)
                ctx.check(getattr(ctx._lib, entry)(ctx.ptr, *lead, *args(o)), entry)
                ctx.synchronize()
                outs.append(o.cpu().numpy())
            assert all(_same(outs[0][ix], outs[1][ix]) for ix in written), (forwarder, pt)
            return outs[1]

        seq = _up(np.stack([q, r]), torch_dev)
        got = both(twin + "_sequence_dev", "nsof_farneback_px_sequence_dev",
                   lambda o: (2, seq.data_ptr(), 200 * px, 72 * 200 * px, 200, 72, o.data_ptr(), *_args(p)), (1, 72, 200, 2))
        assert _same(got[0], f_tw), pt

        def dev_list(o):   # the whole pair and a crop of it (rows 5..60, columns 8..136), each into its own canvas
            descs = (_lib.PairDesc * 2)()
            for i, (y0, y1, x0, x1) in enumerate(((0, 72, 0, 200), (5, 60, 8, 136))):
                d = descs[i]
                d.prev, d.next = tq[y0:y1, x0:x1].data_ptr(), tr[y0:y1, x0:x1].data_ptr()
                d.prev_stride = d.next_stride = 200 * px
                d.width, d.height, d.flow, d.flow_stride = x1 - x0, y1 - y0, o[i, y0:y1, x0:x1].data_ptr(), 1600
            return (2, descs, *_args(p))
        got = both(twin + "_batch_desc_dev", "nsof_farneback_px_batch_desc_dev", dev_list, (2, 72, 200, 2),
                   written=((0,), (1, slice(5, 60), slice(8, 136))))
        assert _same(got[0], f_tw), pt
        assert not (got[1, 5:60, 8:136] == 1.0).all(), "the crop was not written"

        hosts = []
        for entry, lead in ((twin + "_batch", ()), ("nsof_farneback_px_batch", (pt,))):
            f = np.full((72, 200, 2), float(len(hosts)), np.float32)
            descs = (_lib.PairDesc * 1)()
            d = descs[0]
            d.prev, d.prev_stride, d.next, d.next_stride = q.ctypes.data, q.strides[0], r.ctypes.data, r.strides[0]
            d.width, d.height, d.flow, d.flow_stride = 200, 72, f.ctypes.data, 1600
            ctx.check(getattr(ctx._lib, entry)(ctx.ptr, *lead, 1, descs, *_args(p)), entry)
            hosts.append(f)
        assert _same(hosts[0], hosts[1]) and _same(hosts[0], f_tw), pt

        counts = torch.tensor([2, 0], dtype=torch.int32, device=torch_dev)   # two overlapping crops of the one pair
        rects = torch.tensor([[[8, 4, 136, 60], [100, 20, 196, 70]], [[0, 0, 0, 0], [0, 0, 0, 0]]], dtype=torch.int32,
                             device=torch_dev)
        got = both(twin + "_roi_sequence_dev", "nsof_farneback_px_roi_sequence_dev",
                   lambda o: (2, seq.data_ptr(), 200 * px, 72 * 200 * px, 200, 72, counts.data_ptr(), rects.data_ptr(), 2,
                              o.data_ptr(), *_args(p), 0, None, None), (1, 72, 200, 2))
        assert got[0, 4:60, 8:136].any() and not got[0, :4].any(), pt

        for level in (0, 1):
            wk, hk = nsof_lib.level_size(200, 72, p.pyr_scale, level)[:2]
            both("nsof_stage_pyr_level" + ("" if pt == _lib.PIXEL_U8 else "_f32"), "nsof_stage_pyr_level_px",
                 lambda o: (1, tq.data_ptr(), 200 * px, 0, 200, 72, p.pyr_scale, level, o.data_ptr()), (hk, wk))   # noqa: B023


# ---- 9. refusals --------------------------------------------------------------------------------------------------
def test_refusals_before_launch(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import _lib
    from nsof.farneback import farneback_pairs_16_dev
    p = PARAM_SETS["A"]
    h, w = 40, 64
    buf = _up(np.zeros((2, h, w + 2), np.int16), torch_dev)
    canvas = torch.full((1, h, w, 2), 7.0, dtype=torch.float32, device=torch_dev)
    base, odd = buf.data_ptr(), buf.data_ptr() + 1
    rs = (w + 2) * 2
    bad = [(_lib.PIXEL_U16, odd, rs), (_lib.PIXEL_S16, base, rs - 1), (_lib.PIXEL_U16, base, 2 * w - 2), (7, base, rs),
           (-1, base, rs)]
    ctx.prof_enable(_lib.K_PREP, _lib.K_POLYEXP, _lib.K_ITERATE)
    try:
        for pt, ptr, stride in bad:
            rc = ctx._lib.nsof_farneback_px_batch_dev(ctx.ptr, pt, 1, ptr, ptr + h * rs, stride, h * rs, w, h,
                                                      canvas.data_ptr(), *_args(p))
            assert rc == _lib.NSOF_EINVAL, (pt, ptr - base, stride)
            rc = ctx._lib.nsof_farneback_px_sequence_dev(ctx.ptr, pt, 2, ptr, stride, h * rs, w, h, canvas.data_ptr(),
                                                         *_args(p))
            assert rc == _lib.NSOF_EINVAL, (pt, ptr - base, stride)
            descs = (_lib.PairDesc * 1)()
            d = descs[0]
            d.prev, d.prev_stride, d.next, d.next_stride = ptr, stride, ptr + h * rs, stride
            d.width, d.height, d.flow, d.flow_stride = w, h, canvas.data_ptr(), w * 8
            assert ctx._lib.nsof_farneback_px_batch_desc_dev(ctx.ptr, pt, 1, descs, *_args(p)) == _lib.NSOF_EINVAL
            out = np.zeros((h, w, 2), np.float32)
            hp = np.zeros((h, w + 2), np.int16)
            assert ctx._lib.nsof_farneback_px(ctx.ptr, pt, hp.ctypes.data + (ptr - base), stride, hp.ctypes.data, stride,
                                              w, h, out.ctypes.data, w * 8, *_args(p)) == _lib.NSOF_EINVAL
        # an odd frame stride
        assert ctx._lib.nsof_farneback_px_batch_dev(ctx.ptr, _lib.PIXEL_U16, 1, base, base + h * rs, rs, h * rs + 1, w, h,
                                                    canvas.data_ptr(), *_args(p)) == _lib.NSOF_EINVAL
        assert ctx._lib.nsof_stage_pyr_level_px(ctx.ptr, 9, 1, base, rs, 0, w, h, 0.5, 0, canvas.data_ptr()) == _lib.NSOF_EINVAL
        launches = [ctx.prof_collect(k)[1] for k in (_lib.K_PREP, _lib.K_POLYEXP, _lib.K_ITERATE)]
    finally:
        ctx.prof_enable()
    assert launches == [0, 0, 0]
    assert bool((canvas == 7.0).all())
    # device lists hold one 16-bit dtype
    u16, s16, u8 = (_up(np.zeros((h, w), dt), torch_dev) for dt in (np.uint16, np.int16, np.uint8))
    for pair in ((u16, s16), (u8, u16), (u8, u8)):
        with pytest.raises(NsofValueError):
            farneback_pairs_16_dev([pair], [canvas[0]], p, ctx=ctx)
    with pytest.raises(NsofValueError):
        farneback_pairs_16_dev([(u16, u16), (s16, s16)], [canvas[0], canvas[0]], p, ctx=ctx)


# ---- layouts at the edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_host_views_flipped_and_unaligned(nsof_lib, ctx, dtype):
    """Views nsof_farneback_px does not take as they are -- a negative row stride, an odd start address -- are copied
    by calcOpticalFlowFarneback, as their astype(np.float32) is: the result is the float32 call's."""
    p = PARAM_SETS["A"]
    a, b = _pair16(6, 64, 200, dtype)
    fa, fb = np.flipud(a), np.flipud(b)
    assert fa.strides[0] < 0
    assert _same(nsof_lib.calcOpticalFlowFarneback(fa, fb, None, *_args(p), ctx=ctx), _f32_flow(nsof_lib, ctx, fa, fb, p))
    raw = np.zeros(2 * a.nbytes + 2, np.uint8)
    ua = np.frombuffer(raw.data, dtype, a.size, offset=1).reshape(a.shape)
    ub = np.frombuffer(raw.data, dtype, b.size, offset=1 + a.nbytes).reshape(b.shape)
    assert ua.ctypes.data % 2 == 1
    ua[...], ub[...] = a, b
    assert _same(nsof_lib.calcOpticalFlowFarneback(ua, ub, None, *_args(p), ctx=ctx), _f32_flow(nsof_lib, ctx, a, b, p))


@pytest.mark.parametrize("dtype", ["uint8"] + DTYPES)
def test_frames_flush_with_their_buffer(nsof_lib, ctx, torch_dev, pyr_fma, dtype):
    """Set A on frames whose first row starts a buffer and whose last row ends one, at widths that take the 8-column
    lanes of the decimating walks (W % 16 == 8; every 16-bit three-level launch), where the 19-tap scale-8 halo is wider
    than a lane: the result is the float32 path's, and the lanes next to the image edges keep their loads in the row."""
    import torch
    from nsof.farneback import farneback_batch, farneback_sequence
    p = PARAM_SETS["A"]
    for (h, w) in ((64, 200), (1080, 1080)):
        a, b = _pair16(13, h, w, "uint16" if dtype == "uint8" else dtype)
        if dtype == "uint8":
            a, b = (np.right_shift(x, 8).astype(np.uint8) for x in (a, b))
        want = torch.empty((1, h, w, 2), dtype=torch.float32, device=torch_dev)
        farneback_batch(_up(a.astype(np.float32), torch_dev), _up(b.astype(np.float32), torch_dev), want, 1, h, w, p, ctx=ctx)
        # prev at the start of its own allocation, next at the end of a larger one
        ta = _up(a, torch_dev)
        big = _up(np.concatenate([np.zeros(5 * w + 8, a.dtype), b.ravel()]), torch_dev)
        tb = big[5 * w + 8:].view(h, w)
        got = torch.empty_like(want)
        farneback_batch(ta, tb, got, 1, h, w, p, ctx=ctx)
        # a two-frame sequence that fills its buffer exactly
        seq = torch.empty_like(want)
        farneback_sequence(_up(np.stack([a, b]), torch_dev), seq, 2, h, w, p, ctx=ctx)
        ctx.synchronize()
        assert _same(got.cpu().numpy(), want.cpu().numpy()), (h, w)
        assert _same(seq.cpu().numpy(), want.cpu().numpy()), (h, w)
