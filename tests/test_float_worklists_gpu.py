"""GPU: float and 16-bit frames in the Farneback work lists (host lists, device lists, the device ROI sequence, the
float surface of the config-3 pipeline).

1. host ``farneback_pairs`` on uint16, int16, float32 and float64 lists: each item equals ``calcOpticalFlowFarneback`` of
   its pair bit for bit (parameter sets A, B, C; exact and fast; both pyramid arithmetic variants), written into canvas
   views;
2. every route of a float list (small-batch form, k_iterate_x's job tables, the uniform driver, per-item fallback,
   several pipeline chunks, page-locked frames and flows, a mixed uint8 + uint16 list) equals the lone calls;
3. a float32 list holding 8-bit values equals the 8-bit list;
4. ``farneback_pairs_f32_dev`` on crops of float frames in HBM (16-byte aligned and odd-element starts);
5. ``farneback_roi_sequence_f32_dev`` against the u8 sequence (8-bit values) and against lone calls pasted in label order;
6. ``events_to_roi_flows(surface_dtype="float32")``;
7. refusals before any launch."""
import numpy as np
import pytest

from nsof.errors import NsofValueError
from test_float_reference import PARAM_SETS, shifted_pair

pytestmark = pytest.mark.gpu

ARGS = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags")


def _args(p):
    return [getattr(p, k) for k in ARGS]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a, np.float32).view(np.int32),
                                                 np.asarray(b, np.float32).view(np.int32))


@pytest.fixture(params=[0, 1], ids=["plain", "fma"])
def pyr_fma(request, ctx):
    from nsof import _lib
    saved = ctx.get_option(_lib.OPT_PYR_FMA)
    ctx.set_option(_lib.OPT_PYR_FMA, request.param)
    yield request.param
    ctx.set_option(_lib.OPT_PYR_FMA, saved)


@pytest.fixture(params=[True, False], ids=["exact", "fast"])
def exact(request, ctx):
    from nsof import _lib
    saved = ctx.get_option(_lib.OPT_EXACT_ROWSUMS)
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 1 if request.param else 0)
    yield request.param
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, saved)


RANGES = {"uint16": (0.0, 65535.0), "int16": (-30000.0, 30000.0), "float32": (-1000.0, 1000.0), "float64": (0.0, 1.0)}
H, W = 120, 404   # W % 4 == 0


def _frames(seed, dtype, h=H, w=W):
    lo, hi = RANGES[np.dtype(dtype).name] if np.dtype(dtype).name in RANGES else (0.0, 255.0)
    a, b = shifted_pair(seed, h, w, lo, hi)
    if np.issubdtype(dtype, np.integer):
        return np.rint(a).astype(dtype), np.rint(b).astype(dtype)
    return a.astype(dtype), b.astype(dtype)


# (y0, y1, x0, x1) of the crops of one list: strip edges (191 / 192 / 193 / 385 columns), odd starts and widths,
# W % 4 == 0 and != 0, a tiny item
CROPS = [(0, H, 0, W), (10, 70, 3, 196), (5, 50, 8, 200), (0, 9, 1, 13), (20, 81, 37, 102), (3, 120, 11, 396),
         (40, 101, 100, 291)]


def _crop_list(a, b):
    pairs = [(a[y0:y1, x0:x1], b[y0:y1, x0:x1]) for (y0, y1, x0, x1) in CROPS]
    pairs.append((a[::2, ::2][:50, :100], b[::2, ::2][:50, :100]))   # non-unit pixel stride: converted
    return pairs


def _check_list(nsof_lib, ctx, pairs, flows, p):
    for i, ((pa, pb), f) in enumerate(zip(pairs, flows)):
        ref = nsof_lib.calcOpticalFlowFarneback(pa, pb, None, *_args(p), ctx=ctx)
        assert _same(f, ref), f"item {i} {pa.shape}"


@pytest.mark.parametrize("dtype", ["uint16", "int16", "float32", "float64"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_host_pairs_equal_lone_calls(nsof_lib, ctx, pyr_fma, exact, name, dtype):
    from nsof.farneback import farneback_pairs
    p = PARAM_SETS[name]
    a, b = _frames(3, np.dtype(dtype))
    pairs = _crop_list(a, b)
    canvases = [np.zeros((H, W, 2), np.float32) for _ in CROPS]
    flows = [c[y0:y1, x0:x1] for c, (y0, y1, x0, x1) in zip(canvases, CROPS)] + [np.empty((50, 100, 2), np.float32)]
    out = farneback_pairs(pairs, p, flows, ctx=ctx)
    assert all(o is f for o, f in zip(out, flows))
    _check_list(nsof_lib, ctx, pairs, flows, p)
    assert np.abs(flows[0]).max() > (0.1 if dtype != "float64" else 0.0)   # [0, 1] frames: near-zero flow, as cv2's
    for c, (y0, y1, x0, x1) in zip(canvases, CROPS):   # nothing written outside the views
        c[y0:y1, x0:x1] = 0
        assert not c.any()


def test_route_small_batch_and_job_tables(nsof_lib, ctx):
    """A short list takes the small-batch form (exact_lat); 40 crops of 200 columns (80 strip jobs) k_iterate_x's tables.
    Both lists on a fresh context: its work-list tables and pipeline slots grow from the short list's to the long one's."""
    from nsof.farneback import farneback_pairs
    p = PARAM_SETS["A"]
    a, b = _frames(5, np.dtype("uint16"))
    small = [(a[0:30, 0:50], b[0:30, 0:50]), (a[7:60, 9:70], b[7:60, 9:70])]
    big = [(a[y:y + 40 + y % 7, x:x + 200], b[y:y + 40 + y % 7, x:x + 200]) for y in range(0, 80, 10)
           for x in (0, 1, 50, 103, 204)]
    assert sum((q[0].shape[1] + 191) // 192 for q in big) > 64
    fresh = nsof_lib.Context(0)
    try:
        _check_list(nsof_lib, ctx, small, farneback_pairs(small, p, ctx=fresh), p)
        _check_list(nsof_lib, ctx, big, farneback_pairs(big, p, ctx=fresh), p)
    finally:
        fresh.close()


def test_route_uniform_fallback_chunks(nsof_lib, ctx, monkeypatch):
    """Equal shapes (the host pipeline packs them at constant strides: the uniform driver); winsize 17 (per-item
    fallback on the f32 core); NSOF_PIPE_CHUNK_MB=1 (several pipeline chunks)."""
    from nsof.farneback import FarnebackParams, farneback_pairs
    p = PARAM_SETS["B"]
    seq = [_frames(20 + i, np.dtype("float32"))[i % 2] for i in range(6)]
    uniform = [(seq[i], seq[i + 1]) for i in range(5)]
    _check_list(nsof_lib, ctx, uniform, farneback_pairs(uniform, p, ctx=ctx), p)
    p17 = FarnebackParams(0.5, 2, 17, 2, 5, 1.1, 0)
    a, b = _frames(6, np.dtype("int16"))
    mixed = [(a, b), (a[3:50, 5:77], b[3:50, 5:77])]
    _check_list(nsof_lib, ctx, mixed, farneback_pairs(mixed, p17, ctx=ctx), p17)
    monkeypatch.setenv("NSOF_PIPE_CHUNK_MB", "1")
    many = [(seq[i % 5], seq[i % 5 + 1]) for i in range(4)] + _crop_list(a, b)
    _check_list(nsof_lib, ctx, many, farneback_pairs(many, p, ctx=ctx), p)


def test_route_pinned_frames_and_flows(nsof_lib, ctx):
    from nsof.farneback import farneback_pairs, pinned_empty
    p = PARAM_SETS["C"]
    pairs = []
    for i, (h, w) in enumerate([(H, W), (64, 130), (33, 192)]):
        a, b = _frames(30 + i, np.dtype("float32"), h, w)
        pa, pb = pinned_empty((h, w), np.float32), pinned_empty((h, w), np.float32)
        pa[...], pb[...] = a, b
        pairs.append((pa, pb))
    flows = farneback_pairs(pairs, p, pinned=True, ctx=ctx)
    _check_list(nsof_lib, ctx, pairs, flows, p)
    pairs16 = [(np.rint((x + 1000) * 30).astype(np.uint16), np.rint((y + 1000) * 30).astype(np.uint16)) for x, y in pairs]
    _check_list(nsof_lib, ctx, pairs16, farneback_pairs(pairs16, p, pinned=True, ctx=ctx), p)


def test_route_conversion_beyond_the_page_locked_cap(nsof_lib, monkeypatch):
    """A list whose conversion does not fit the context's page-locked buffer: the rest goes through ordinary arrays;
    close() releases the buffer."""
    import nsof
    from nsof import farneback as F
    monkeypatch.setattr(F, "_F32_STAGE_CAP", 256 << 10)
    p = PARAM_SETS["A"]
    a, b = _frames(14, np.dtype("uint16"))
    pairs = [(a, b)] + _crop_list(a, b) + [(a, b)]   # > 256 KiB of float32 frames
    with nsof.Context(0) as c:
        flows = F.farneback_pairs(pairs, p, ctx=c)
        assert c._nsof_f32_stage.nbytes == 256 << 10
        _check_list(nsof_lib, c, pairs, flows, p)
    assert "_nsof_f32_stage" not in c.__dict__


def test_route_mixed_u8_and_u16_list(nsof_lib, ctx, pyr_fma):
    from nsof import synth
    from nsof.farneback import farneback_pairs
    p = PARAM_SETS["A"]
    u8 = synth.make_pair(4, 90, 150)
    a, b = _frames(8, np.dtype("uint16"))
    pairs = [u8, (a[0:70, 1:140], b[0:70, 1:140]), (u8[0][10:60, 3:100], u8[1][10:60, 3:100])]
    _check_list(nsof_lib, ctx, pairs, farneback_pairs(pairs, p, ctx=ctx), p)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_f32_list_of_u8_values_is_u8_list(nsof_lib, ctx, pyr_fma, exact, name):
    from nsof import synth
    from nsof.farneback import farneback_pairs
    p = PARAM_SETS[name]
    a, b = synth.make_pair(9, H, W)
    pairs = _crop_list(a, b)
    want = farneback_pairs(pairs, p, ctx=ctx)
    got = farneback_pairs([(x.astype(np.float32), y.astype(np.float32)) for x, y in pairs], p, ctx=ctx)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert _same(g, w_), i


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_pairs_on_crops_in_hbm(nsof_lib, ctx, torch_dev, pyr_fma, name):
    import torch
    from nsof.farneback import farneback_pairs_f32_dev
    p = PARAM_SETS[name]
    a, b = _frames(11, np.dtype("float32"))
    ta, tb = torch.from_numpy(a).to(torch_dev), torch.from_numpy(b).to(torch_dev)
    assert ta.data_ptr() % 16 == 0 and (W * 4) % 16 == 0
    # x0 % 4 == 0 with W % 4 == 0: rows start 16-byte aligned (vector level 0); odd x0: scalar level 0
    crops = [(0, H, 0, W), (8, 72, 4, 200), (5, 60, 16, 216), (10, 70, 3, 196), (0, 9, 1, 13), (20, 81, 37, 102)]
    canvas = torch.zeros((len(crops), H, W, 2), dtype=torch.float32, device=torch_dev)
    pairs = [(ta[y0:y1, x0:x1], tb[y0:y1, x0:x1]) for (y0, y1, x0, x1) in crops]
    flows = [canvas[i, y0:y1, x0:x1] for i, (y0, y1, x0, x1) in enumerate(crops)]
    farneback_pairs_f32_dev(pairs, flows, p, ctx=ctx)
    ctx.synchronize()
    host = canvas.cpu().numpy()
    for i, (y0, y1, x0, x1) in enumerate(crops):
        ref = nsof_lib.calcOpticalFlowFarneback(a[y0:y1, x0:x1], b[y0:y1, x0:x1], None, *_args(p), ctx=ctx)
        assert _same(host[i, y0:y1, x0:x1], ref), (y0, y1, x0, x1)
        host[i, y0:y1, x0:x1] = 0
        assert not host[i].any()
    # a uniform device list (consecutive frames, dense flows): the uniform driver
    seq = torch.from_numpy(np.stack([_frames(40 + k, np.dtype("float32"))[k % 2] for k in range(4)])).to(torch_dev)
    fl = torch.empty((3, H, W, 2), dtype=torch.float32, device=torch_dev)
    farneback_pairs_f32_dev([(seq[k], seq[k + 1]) for k in range(3)], [fl[k] for k in range(3)], p, ctx=ctx)
    ctx.synchronize()
    s, fl = seq.cpu().numpy(), fl.cpu().numpy()
    for k in range(3):
        assert _same(fl[k], nsof_lib.calcOpticalFlowFarneback(s[k], s[k + 1], None, *_args(p), ctx=ctx)), k


# per frame: rectangles (x0, y0, x1, y1); FLAG 1 style boxes that overlap, an empty one, a full-frame one
ROI_TABLE = [[(10, 5, 140, 90), (100, 40, 300, 118), (0, 0, 0, 0), (290, 2, 404, 60)],
             [(0, 0, 404, 120), (51, 13, 120, 99)],
             [(3, 3, 15, 12), (200, 20, 395, 111), (250, 60, 330, 100)],
             [(7, 9, 230, 80)]]


def _roi_tensors(torch_dev):
    import torch
    n, m = len(ROI_TABLE), max(len(r) for r in ROI_TABLE)
    counts = torch.tensor([len(r) for r in ROI_TABLE], dtype=torch.int32, device=torch_dev)
    rects = np.zeros((n, m, 4), np.int32)
    for k, rs in enumerate(ROI_TABLE):
        rects[k, :len(rs)] = rs
    return counts, torch.from_numpy(rects).to(torch_dev)


def _roi_reference(nsof_lib, ctx, frames, p, gate_frame):
    out = np.zeros((len(frames) - 1, H, W, 2), np.float32)
    for k in range(len(frames) - 1):
        for (x0, y0, x1, y1) in ROI_TABLE[k + gate_frame]:
            if x1 > x0 and y1 > y0:
                out[k, y0:y1, x0:x1] = nsof_lib.calcOpticalFlowFarneback(frames[k][y0:y1, x0:x1], frames[k + 1][y0:y1, x0:x1],
                                                                         None, *_args(p), ctx=ctx)
    return out


@pytest.mark.parametrize("gate_frame", [0, 1])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_roi_sequence_f32(nsof_lib, ctx, torch_dev, name, gate_frame):
    import torch
    from nsof import synth
    from nsof.farneback import farneback_roi_sequence_dev, farneback_roi_sequence_f32_dev
    p = PARAM_SETS[name]
    counts, rects = _roi_tensors(torch_dev)
    n = len(ROI_TABLE)
    # 8-bit values: the float sequence equals the u8 sequence
    u8 = np.stack([synth.make_pair(12 + k // 2, H, W)[k % 2] for k in range(n)])
    tu = torch.from_numpy(u8).to(torch_dev)
    fu = torch.empty((n - 1, H, W, 2), dtype=torch.float32, device=torch_dev)
    cu = farneback_roi_sequence_dev(tu, counts, rects, fu, p, gate_frame=gate_frame, ctx=ctx)
    # padded rows: the frames' row stride is free
    pad = torch.full((n, H, W + 3), -5.0, dtype=torch.float32, device=torch_dev)
    pad[:, :, :W] = tu.float()
    ff = torch.empty((n - 1, H, W, 2), dtype=torch.float32, device=torch_dev)
    cf = farneback_roi_sequence_f32_dev(pad[:, :, :W], counts, rects, ff, p, gate_frame=gate_frame, ctx=ctx)
    ctx.synchronize()
    assert cf == cu and cf[0] >= 3
    assert _same(ff.cpu().numpy(), fu.cpu().numpy())
    # general float frames: every crop is the lone float call, pasted in label order (later boxes win)
    fr = np.stack([_frames(50 + k // 2, np.dtype("float32"))[k % 2] for k in range(n)])
    g = torch.empty((n - 1, H, W, 2), dtype=torch.float32, device=torch_dev)
    farneback_roi_sequence_f32_dev(torch.from_numpy(fr).to(torch_dev), counts, rects, g, p, gate_frame=gate_frame, ctx=ctx)
    ctx.synchronize()
    assert _same(g.cpu().numpy(), _roi_reference(nsof_lib, ctx, fr, p, gate_frame))


def test_events_to_roi_flows_float_surface(nsof_lib, ctx):
    from nsof import gating, pipeline, synth
    from nsof.farneback import PARAMS_B
    Hs, Ws, every = 240, 320, 40   # noqa: N806
    x, y, pol, t = synth.make_events(7, Ws, Hs, n_background=3000, duration_us=160_000, box=(40, 30), speed_pps=500.0)
    for flag in (1, 2):
        cfg = gating.GatingConfig(MEMSIZE=20, EXTEND_HEIGHT_UPPER=10, EXTEND_HEIGHT_LOWER=10, EXTEND_WIDTH_LEFT=10,
                                  EXTEND_WIDTH_RIGHT=10, THRES=240, FLAG=flag, farneback_params=PARAMS_B)
        kw = dict(slice_us=1000, silent_v=0.5, snapshot_every=every, ctx=ctx)
        _, rects_u8, _ = pipeline.events_to_roi_flows(x, y, pol, t, (Hs, Ws), cfg, **kw)
        tm = {}
        frames, rects, flows = pipeline.events_to_roi_flows(x, y, pol, t, (Hs, Ws), cfg, surface_dtype="float32", timings=tm,
                                                            **kw)
        assert str(frames.dtype) == "torch.float32" and rects == rects_u8 and tm["roi_calls"] >= 1
        fr, fl = frames.cpu().numpy(), flows.cpu().numpy()
        assert (np.abs(fr - np.round(fr)) > 1e-4).any()   # unquantised surface values
        for k in range(fr.shape[0] - 1):
            want = np.zeros((Hs, Ws, 2), np.float32)
            for (x0, y0, x1, y1) in rects[k]:   # bug-compatible gating: the map of the pair's first frame
                want[y0:y1, x0:x1] = nsof_lib.calcOpticalFlowFarneback(fr[k][y0:y1, x0:x1], fr[k + 1][y0:y1, x0:x1], None,
                                                                       *_args(PARAMS_B), ctx=ctx)
            assert _same(fl[k], want), (flag, k)
        assert any(len(r) for r in rects[:-1])
    with pytest.raises(ValueError):
        pipeline.events_to_roi_flows(x, y, pol, t, (Hs, Ws), cfg, surface_dtype="float16", **kw)


def test_refusals_before_launch(nsof_lib, ctx, torch_dev):
    import ctypes as C
    import torch
    import nsof
    from nsof import _lib
    from nsof.farneback import farneback_pairs, farneback_pairs_f32_dev, farneback_roi_sequence_f32_dev
    p = PARAM_SETS["A"]
    a, b = _frames(2, np.dtype("float32"), 40, 64)
    ta, tb = torch.from_numpy(a).to(torch_dev), torch.from_numpy(b).to(torch_dev)
    flow = torch.zeros((40, 64, 2), dtype=torch.float32, device=torch_dev)
    # misaligned pointer / stride -> nsof.error from the C layer
    descs = (_lib.PairDesc * 1)()
    d = descs[0]
    d.prev, d.prev_stride, d.next, d.next_stride = ta.data_ptr() + 2, 256, tb.data_ptr(), 256
    d.width, d.height, d.flow, d.flow_stride = 60, 40, flow.data_ptr(), 64 * 8
    with pytest.raises(nsof.error):
        ctx.check(ctx._lib.nsof_farneback_f32_batch_desc_dev(ctx.ptr, 1, descs, *_args(p)), "f32 desc")
    d.prev, d.prev_stride = ta.data_ptr(), 254
    with pytest.raises(nsof.error):
        ctx.check(ctx._lib.nsof_farneback_f32_batch_desc_dev(ctx.ptr, 1, descs, *_args(p)), "f32 desc")
    d.prev_stride = 200   # < 4 * width
    with pytest.raises(nsof.error):
        ctx.check(ctx._lib.nsof_farneback_f32_batch_desc_dev(ctx.ptr, 1, descs, *_args(p)), "f32 desc")
    host = (_lib.PairDesc * 1)()
    ha = np.zeros((40, 65), np.float32)
    hf = np.zeros((40, 64, 2), np.float32)
    h = host[0]
    h.prev, h.prev_stride, h.next, h.next_stride = ha.ctypes.data, 258, ha.ctypes.data, 260
    h.width, h.height, h.flow, h.flow_stride = 64, 40, hf.ctypes.data, 64 * 8
    with pytest.raises(nsof.error):
        ctx.check(ctx._lib.nsof_farneback_f32_batch(ctx.ptr, 1, host, *_args(p)), "f32 host")
    counts = torch.ones(2, dtype=torch.int32, device=torch_dev)
    rects = torch.tensor([[[0, 0, 8, 8]], [[0, 0, 8, 8]]], dtype=torch.int32, device=torch_dev)
    frames = torch.stack([ta, tb])
    flows = torch.zeros((1, 40, 64, 2), dtype=torch.float32, device=torch_dev)
    calls, pixels = C.c_longlong(), C.c_longlong()
    rc = ctx._lib.nsof_farneback_f32_roi_sequence_dev(ctx.ptr, 2, frames.data_ptr(), 258, 40 * 258, 64, 40, counts.data_ptr(),
                                                      rects.data_ptr(), 1, flows.data_ptr(), *_args(p), 0, C.byref(calls),
                                                      C.byref(pixels))
    with pytest.raises(nsof.error):
        ctx.check(rc, "f32 roi")
    # other dtypes to the _f32_dev functions
    with pytest.raises(NsofValueError):
        farneback_pairs_f32_dev([(ta.double(), tb.double())], [flow], p, ctx=ctx)
    with pytest.raises(NsofValueError):
        farneback_pairs_f32_dev([((ta * 100).to(torch.uint8), (tb * 100).to(torch.uint8))], [flow], p, ctx=ctx)
    with pytest.raises(NsofValueError):
        farneback_roi_sequence_f32_dev(frames.double(), counts, rects, flows, p, ctx=ctx)
    with pytest.raises(NsofValueError):
        farneback_roi_sequence_f32_dev(frames.to(torch.uint8), counts, rects, flows, p, ctx=ctx)
    ctx.synchronize()
    # host lists: non-finite values, dtypes differing within a pair
    for bad in (np.nan, np.inf, -np.inf):
        c = b.copy()
        c[3, 4] = bad
        with pytest.raises(NsofValueError):
            farneback_pairs([(a, b), (a, c)], p, ctx=ctx)
    with pytest.raises(NsofValueError):
        farneback_pairs([(a, b), (a.astype(np.float64), np.full((40, 64), 1e39))], p, ctx=ctx)
    with pytest.raises(NsofValueError):
        farneback_pairs([(a, b.astype(np.uint16))], p, ctx=ctx)
