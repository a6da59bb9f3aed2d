"""GPU: Farneback on float32 frames (and the other depths cv2 accepts), the float pyramid stage, the float surface.

1. float32 frames holding 8-bit values give the 8-bit path's flow bit for bit (lone, batch, sequence; both pyramid
   arithmetic variants; exact and fast mode; the three-level, decimating and walking pyramid launches; strip-edge, odd
   and tiny widths; strided and element-offset crops);
2. general float frames give the CPU float reference of tests/test_float_reference.py bit for bit (default variant,
   exact mode);
3. nsof_stage_pyr_level_f32 equals the NumPy blur + oracle.resize_linear at every level;
4. every accepted dtype equals the float32 call on its astype(np.float32); rejected inputs raise before device work;
5. torch float32 tensors dispatch to the float entries, work lists refuse them;
6. Accumulator.surface_f32: its values, its relation to surface_u8, and events -> float surface -> flow sequence."""
import numpy as np
import pytest

from nsof.errors import NsofValueError
from test_float_reference import PARAM_SETS, blur_f32, farneback_f32, shifted_pair, smooth_field

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


def _pair_u8(seed, h, w):
    from nsof import synth
    return synth.make_pair(seed, h, w)


# (param set, height, width): pyr_scale 0.5 on widths that take the three-level launch (u8) / the 16- and 8-column
# decimating walks (f32), generic scales (walking kernel), the 192-column strip edges of the iteration, odd and tiny
LONE_CASES = [("A", 96, 256), ("A", 72, 200), ("A", 61, 191), ("B", 64, 192), ("C", 50, 193), ("B", 45, 385),
              ("C", 17, 23), ("A", 9, 12), ("B", 31, 7)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
@pytest.mark.parametrize("name,h,w", LONE_CASES)
def test_f32_of_u8_values_is_u8_flow_lone(nsof_lib, ctx, pyr_fma, exact, name, h, w):
    p = PARAM_SETS[name]
    a, b = _pair_u8(3, h, w)
    ref = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx, exact=exact)
    got = nsof_lib.calcOpticalFlowFarneback(a.astype(np.float32), b.astype(np.float32), None, *_args(p), ctx=ctx,
                                            exact=exact)
    assert _same(got, ref)


def _set_exact(ctx, exact):
    from nsof import _lib
    saved = ctx.get_option(_lib.OPT_EXACT_ROWSUMS)
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 1 if exact else 0)
    return saved


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "fast"])
@pytest.mark.parametrize("n,name,h,w", [(1, "A", 96, 256), (3, "B", 61, 193), (70, "A", 40, 64), (5, "C", 33, 200)])
def test_f32_of_u8_values_is_u8_flow_batch_and_sequence(nsof_lib, ctx, torch_dev, pyr_fma, exact, n, name, h, w):
    import torch
    from nsof import _lib
    from nsof.farneback import farneback_batch, farneback_sequence
    p = PARAM_SETS[name]
    frames = np.stack([_pair_u8(10 + i // 2, h, w)[i % 2] for i in range(n + 1)])
    # crops of larger frames: an odd element offset and padded rows (strided, unaligned starts)
    big = np.zeros((n + 1, h + 5, w + 7), np.uint8)
    big[:, 2:2 + h, 3:3 + w] = frames
    tu = torch.from_numpy(big).to(torch_dev)
    tf = tu.float()
    cu, cf = tu[:, 2:2 + h, 3:3 + w], tf[:, 2:2 + h, 3:3 + w]
    saved = _set_exact(ctx, exact)
    try:
        outs = {}
        for tag, t, isz in (("u8", cu, 1), ("f32", cf, 4)):
            fb = torch.empty((n, h, w, 2), dtype=torch.float32, device=torch_dev)
            farneback_batch(t[:-1], t[1:], fb, n, h, w, p, row_stride=t.stride(1) * isz, pair_stride=t.stride(0) * isz,
                            ctx=ctx)
            fs = torch.empty((n, h, w, 2), dtype=torch.float32, device=torch_dev)
            farneback_sequence(t, fs, n + 1, h, w, p, row_stride=t.stride(1) * isz, frame_stride=t.stride(0) * isz,
                               ctx=ctx)
            ctx.synchronize()
            outs[tag] = (fb.cpu().numpy(), fs.cpu().numpy())
        # dense float32 frames with the default (dense) strides
        fd = torch.empty((n, h, w, 2), dtype=torch.float32, device=torch_dev)
        dense = tf[:, 2:2 + h, 3:3 + w].contiguous()
        farneback_batch(dense[:-1].contiguous(), dense[1:].contiguous(), fd, n, h, w, p, ctx=ctx)
        ctx.synchronize()
    finally:
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, saved)
    assert _same(outs["f32"][0], outs["u8"][0]), "batch"
    assert _same(outs["f32"][1], outs["u8"][1]), "sequence"
    assert _same(fd.cpu().numpy(), outs["u8"][0]), "dense batch"
    if n <= 5:   # and each pair is the lone call
        for i in range(n):
            ref = nsof_lib.calcOpticalFlowFarneback(frames[i], frames[i + 1], None, *_args(p), ctx=ctx, exact=exact)
            assert _same(outs["f32"][0][i], ref)


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1000.0, 1000.0), (0.0, 65535.0)], ids=["unit", "pm1000", "u16"])
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_general_float_frames_equal_cpu_reference(nsof_lib, ctx, oracle, torch_dev, name, lo, hi):
    import torch
    from nsof import _lib
    from nsof.farneback import farneback_batch, farneback_sequence
    p = PARAM_SETS[name]
    h, w = 72, 104
    a, b = shifted_pair(7, h, w, lo, hi)
    c = shifted_pair(8, h, w, lo, hi)[1]
    saved = _set_exact(ctx, True)
    try:
        ref_ab = farneback_f32(oracle, a, b, *_args(p))
        ref_bc = farneback_f32(oracle, b, c, *_args(p))
        lone = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx)
        t = torch.from_numpy(np.stack([a, b, c])).to(torch_dev)
        fb = torch.empty((2, h, w, 2), dtype=torch.float32, device=torch_dev)
        farneback_batch(t[:2], t[1:], fb, 2, h, w, p, ctx=ctx)
        fs = torch.empty((2, h, w, 2), dtype=torch.float32, device=torch_dev)
        farneback_sequence(t, fs, 3, h, w, p, ctx=ctx)
        ctx.synchronize()
    finally:
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, saved)
    assert _same(lone, ref_ab)
    fb, fs = fb.cpu().numpy(), fs.cpu().numpy()
    assert _same(fb[0], ref_ab) and _same(fb[1], ref_bc)
    assert _same(fs[0], ref_ab) and _same(fs[1], ref_bc)
    # not two zero fields: the wide ranges track the shift; in [0, 1] the solve's + 1e-3 regularisation dominates the
    # tiny determinants and the flow stays near zero (as cv2's does) -- compared bit for bit all the same
    assert np.abs(ref_ab).max() > (0.1 if hi - lo >= 1000 else 0.0)


def test_general_float_1080p_equals_cpu_reference(nsof_lib, ctx, oracle):
    p = PARAM_SETS["A"]
    a, b = shifted_pair(21, 1080, 1920, 0.0, 1.0)
    ref = farneback_f32(oracle, a, b, *_args(p))
    got = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx, exact=True)
    assert _same(got, ref)


@pytest.mark.parametrize("name,h,w", [("A", 96, 256), ("B", 77, 131), ("C", 64, 200), ("A", 1080, 1920)])
@pytest.mark.parametrize("crop", [False, True], ids=["dense", "crop"])
def test_stage_pyr_level_f32_equals_numpy_blur_resize(nsof_lib, ctx, oracle, torch_dev, name, h, w, crop):
    import ctypes as C
    import torch
    p = PARAM_SETS[name]
    img = smooth_field(4, h, w, -50.0, 300.0)
    if crop:   # an element-offset view with padded rows: only 4-byte alignment
        big = np.zeros((h + 2, w + 3), np.float32)
        big[1:1 + h, 1:1 + w] = img
        tb = torch.from_numpy(big).to(torch_dev)
        src = tb[1:1 + h, 1:1 + w]
    else:
        src = torch.from_numpy(img).to(torch_dev)
    L = oracle.effective_levels(w, h, p.pyr_scale, p.levels)
    for k in range(L + 1):
        wk, hk, ks, sg = oracle.level_geometry(w, h, p.pyr_scale, k)
        out = torch.empty((hk, wk), dtype=torch.float32, device=torch_dev)
        rc = ctx._lib.nsof_stage_pyr_level_f32(ctx.ptr, 1, C.c_void_p(src.data_ptr()), src.stride(0) * 4, 0, w, h,
                                               p.pyr_scale, k, C.c_void_p(out.data_ptr()))
        ctx.check(rc, "stage_pyr_level_f32")
        ctx.synchronize()
        ref = oracle.resize_linear(blur_f32(img, ks, sg, oracle.gaussian_kernel), wk, hk)
        assert _same(out.cpu().numpy(), ref), f"level {k}"


ACCEPTED = [np.uint8, np.int8, np.uint16, np.int16, np.int32, np.float16, np.float32, np.float64]


@pytest.mark.parametrize("dt", ACCEPTED, ids=[np.dtype(d).name for d in ACCEPTED])
def test_every_accepted_dtype_is_its_float32_call(nsof_lib, ctx, dt):
    p = PARAM_SETS["A"]
    h, w = 48, 80
    info = np.iinfo(dt) if np.issubdtype(dt, np.integer) else None
    lo, hi = (float(max(info.min, -30000)), float(min(info.max, 40000))) if info else (-3.0, 7.0)
    a, b = shifted_pair(5, h, w, lo, hi)
    a, b = a.astype(dt), b.astype(dt)
    got = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx)
    want = nsof_lib.calcOpticalFlowFarneback(a.astype(np.float32), b.astype(np.float32), None, *_args(p), ctx=ctx)
    assert _same(got, want)
    # the same frames as single-channel (h, w, 1) arrays and as strided views
    assert _same(nsof_lib.calcOpticalFlowFarneback(a[:, :, None], b[:, :, None], None, *_args(p), ctx=ctx), want)
    wide_a, wide_b = np.zeros((h, 2 * w), dt), np.zeros((h, 2 * w), dt)
    wide_a[:, ::2], wide_b[:, ::2] = a, b
    assert _same(nsof_lib.calcOpticalFlowFarneback(wide_a[:, ::2], wide_b[:, ::2], None, *_args(p), ctx=ctx), want)


@pytest.mark.parametrize("case", ["mixed", "bool", "int64", "uint32", "uint64", "complex", "nan", "inf", "f64_overflow"])
def test_rejected_float_inputs_raise(nsof_lib, ctx, case):
    p = PARAM_SETS["A"]
    a = np.full((16, 24), 3, np.float32)
    b = a.copy()
    if case == "mixed":
        b = b.astype(np.uint16)
    elif case in ("bool", "int64", "uint32", "uint64"):
        a, b = a.astype(case), b.astype(case)
    elif case == "complex":
        a, b = a.astype(np.complex64), b.astype(np.complex64)
    elif case == "nan":
        b[3, 4] = np.nan
    elif case == "inf":
        a, b = a.astype(np.float64), b.astype(np.float64)
        a[0, 0] = -np.inf
    elif case == "f64_overflow":   # finite in float64, inf after the conversion to float32
        a, b = a.astype(np.float64), b.astype(np.float64)
        b[1, 1] = 1e39
    with pytest.raises(NsofValueError):
        nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx)


def test_torch_float32_dispatch_and_work_lists_refuse_float(nsof_lib, ctx, torch_dev):
    import torch
    from nsof.farneback import farneback_batch, farneback_pairs_dev, farneback_roi_sequence_dev
    p = PARAM_SETS["B"]
    h, w = 40, 56
    a, b = shifted_pair(2, h, w, 0.0, 1.0)
    ta, tb = torch.from_numpy(a).to(torch_dev), torch.from_numpy(b).to(torch_dev)
    flow = torch.empty((1, h, w, 2), dtype=torch.float32, device=torch_dev)
    farneback_batch(ta, tb, flow, 1, h, w, p, ctx=ctx)          # float32 tensors: the f32 entry, strides 4 * w
    flow_raw = torch.empty_like(flow)
    farneback_batch(ta.data_ptr(), tb.data_ptr(), flow_raw, 1, h, w, p, dtype=np.float32, ctx=ctx)   # raw addresses
    ctx.synchronize()
    want = nsof_lib.calcOpticalFlowFarneback(a, b, None, *_args(p), ctx=ctx)
    assert _same(flow[0].cpu().numpy(), want) and _same(flow_raw[0].cpu().numpy(), want)
    with pytest.raises(NsofValueError):   # other tensor dtypes
        farneback_batch(ta.double(), tb.double(), flow, 1, h, w, p, ctx=ctx)
    with pytest.raises(NsofValueError):   # work lists stay 8-bit
        farneback_pairs_dev([(ta, tb)], [flow[0]], p, ctx=ctx)
    frames = torch.stack([ta, tb])
    counts = torch.zeros(2, dtype=torch.int32, device=torch_dev)
    rects = torch.zeros((2, 4, 4), dtype=torch.int32, device=torch_dev)
    with pytest.raises(NsofValueError):
        farneback_roi_sequence_dev(frames, counts, rects, torch.zeros((1, h, w, 2), device=torch_dev), p, ctx=ctx)


def _surface_ref(oracle, w, mode):
    """float64 evaluation of the surface map on the read-back state (include/nsof.h, nsof_accum_surface_u8_dev)."""
    if mode == "state":
        g = (w.astype(np.float32) * np.float32(255.0)).astype(np.float64)
    else:
        r = oracle.accum_resistance(w).astype(np.float64)
        g = -3366.0 / np.log10(1.0 / r) - 306.0
    return np.clip(g, 0.0, 255.0)


@pytest.mark.parametrize("mode", ["state", "current"])
def test_surface_f32_values(nsof_lib, ctx, oracle, torch_dev, mode):
    import torch
    from nsof import synth
    from nsof.accumulator import Accumulator, slice_index_array
    H, W = 90, 130
    x, y, pol, t = synth.make_events(9, W, H, 6000, 80_000, box=(24, 18))
    idx = slice_index_array(t, 1000)
    acc = Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx)
    try:
        acc.step(x, y, pol, t, idx, snap_every=0)
        wst = acc.w(0)
        f = torch.full((H, W + 3), -1.0, dtype=torch.float32, device=torch_dev)   # padded rows: stride in bytes
        acc.surface_f32(f, 0, row_stride=(W + 3) * 4, mode=mode)
        u = torch.zeros((H, W), dtype=torch.uint8, device=torch_dev)
        acc.surface_u8(u, 0, mode=mode)
        ctx.synchronize()
    finally:
        acc.close()
    f, u = f.cpu().numpy(), u.cpu().numpy()
    assert np.all(f[:, W:] == -1.0)   # nothing written past the row
    f = f[:, :W]
    assert np.isfinite(f).all() and f.min() >= 0 and f.max() <= 255
    assert np.abs(f.astype(np.float64) - _surface_ref(oracle, wst, mode)).max() <= 1e-4
    off_int = np.abs(f - np.round(f)) > 1e-4
    assert np.array_equal(np.floor(f[off_int]).astype(np.uint8), u[off_int])
    assert off_int.any() or mode == "current"


def test_events_to_float_surface_to_flow_sequence(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import synth
    from nsof.accumulator import Accumulator, slice_index_array
    from nsof.farneback import farneback_sequence
    p = PARAM_SETS["A"]
    H, W, n = 96, 160, 4
    x, y, pol, t = synth.make_events(13, W, H, 30000, 400_000, box=(30, 20))
    idx = slice_index_array(t, 1000)
    per = (len(idx) - 1) // n
    frames = torch.empty((n, H, W), dtype=torch.float32, device=torch_dev)
    acc = Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx)
    try:
        for k in range(n):
            acc.step(x, y, pol, t, idx[k * per:(k + 1) * per + 1], snap_every=0)
            acc.surface_f32(frames[k], 0, mode="state")
        flows = torch.empty((n - 1, H, W, 2), dtype=torch.float32, device=torch_dev)
        farneback_sequence(frames, flows, n, H, W, p, ctx=ctx)
        ctx.synchronize()
    finally:
        acc.close()
    host = frames.cpu().numpy()
    assert len({float(np.abs(host[k] - host[k + 1]).sum()) for k in range(n - 1)} - {0.0}) >= 1   # the surface moves
    flows = flows.cpu().numpy()
    for k in range(n - 1):
        ref = nsof_lib.calcOpticalFlowFarneback(host[k], host[k + 1], None, *_args(p), ctx=ctx)
        assert _same(flows[k], ref), f"pair {k}"
