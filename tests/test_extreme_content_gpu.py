"""GPU: degenerate and extreme content, and non-finite flows and maps, against the oracle bit for bit.

1. The matrix update with NaN, +-inf and +-1e10 flows at interior and border pixels: the device's cvFloor returns what
   the oracle's returns (x86 cv2: INT_MIN for NaN and v >= 2^31, INT_MAX below -2^31), so such a sample takes the
   out-of-image branch on both sides and M channels 0-2 stay finite.  A bare float -> int conversion gives 0 for NaN
   on the device and fails here.
2. The remap and the region prediction with the same values in maps and flows, both border modes: x86 cvRound gives
   INT_MIN for all of them (the sample lands left of / above the source).
3. Whole-pipeline content where kernels go wrong -- constant frames, 0/255 checkerboards and step edges, uniform 8-bit
   and full-range 16-bit noise, all-negative float frames, float frames at the scales where the flow turns partly
   and wholly NaN, motions larger than the coarsest level follows -- through the lone call (small-batch form),
   k_iterate_x (OPT_SMALL_BATCH_JOBS = 0), the unfused path (winsize 17), the host work list (every dtype) and, for
   the dtypes they take (uint8, float32), the device work list and the device ROI sequence; NaN positions must match.
   Fast mode: its pipeline tolerance plus the same NaN mask, on every content whose oracle flow is finite.
4. The other heads on the non-finite flows of 1: the motion mask (host call, device call, sequence over boxes) against
   the oracle (a NaN magnitude is not above the threshold, an infinite one is), and the device colour coding against
   its definition for non-finite flows (nsof/flowviz.py flow_to_image_dev): NumPy's coding has no answer there."""
import numpy as np
import pytest

from test_farneback_gpu import PIPE_TOL, _dev, _rlayout
from test_farneback_f64 import translated_pair
from test_float_reference import PARAM_SETS, farneback_f32, shifted_pair
from test_nonfinite_cpu import REMAP_BAD, _flows

pytestmark = pytest.mark.gpu

ARGS = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags")


def _args(p, **over):
    a = {k: getattr(p, k) for k in ARGS}
    a.update(over)
    return [a[k] for k in ARGS]


def _bits_equal(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True) and \
        np.array_equal(np.signbit(got[got == 0]), np.signbit(want[got == 0]))


# ---------------------------------------------------------------- 1. matrix update
@pytest.mark.parametrize("shape", [(23, 31), (12, 70)])
def test_update_matrices_nonfinite_flows(ctx, oracle, torch_dev, shape):
    import torch
    h, w = shape
    img = (np.random.default_rng(2).random((h, w)) * 255).astype(np.float32)
    R0 = oracle.polyexp(img, 5, 1.1)
    R1 = oracle.polyexp(np.roll(img, 2, axis=0), 5, 1.1)
    flow = _flows(h, w)
    want = oracle.update_matrices(R0, R1, flow)
    assert np.isfinite(want[..., :3]).all()
    dR = _dev(torch_dev, np.stack([_rlayout(R0), _rlayout(R1)])[None])
    dF = _dev(torch_dev, flow[None])
    out = torch.empty((1, 5, h, w), dtype=torch.float32, device=torch_dev)
    ctx.check(ctx._lib.nsof_stage_update_matrices(ctx.ptr, 1, dR.data_ptr(), dF.data_ptr(), w, h, out.data_ptr()))
    ctx.synchronize()
    got = np.moveaxis(out.cpu().numpy()[0], 0, -1)
    for c in range(5):
        assert _bits_equal(got[..., c], want[..., c]), f"channel {c}: {np.isnan(got[..., c]).sum()} NaN on the device"


def test_iterate_nonfinite_flows(ctx, oracle, torch_dev):
    """The fused iteration samples through the same floor: the flow after one step equals the oracle's unfused step."""
    import torch
    h, w = 23, 31
    img = (np.random.default_rng(4).random((h, w)) * 255).astype(np.float32)
    R0 = oracle.polyexp(img, 5, 1.1)
    R1 = oracle.polyexp(np.roll(img, 1, axis=1), 5, 1.1)
    flow = _flows(h, w)
    M = oracle.update_matrices(R0, R1, flow)
    dR = _dev(torch_dev, np.stack([_rlayout(R0), _rlayout(R1)])[None])
    dF = _dev(torch_dev, flow[None])
    out = torch.zeros((1, h, w, 2), dtype=torch.float32, device=torch_dev)
    for ws in (3, 15):
        want, _ = oracle.update_flow_blur(R0, R1, flow, M, ws, False)
        ctx.check(ctx._lib.nsof_stage_iterate(ctx.ptr, 1, dR.data_ptr(), dF.data_ptr(), w, h, ws, out.data_ptr()))
        ctx.synchronize()
        assert _bits_equal(out.cpu().numpy()[0], want), ws


# ---------------------------------------------------------------- 2. remap and region prediction
@pytest.mark.parametrize("border", [0, 1])
@pytest.mark.parametrize("cn", [1, 3])
def test_remap_nonfinite_maps(oracle, nsof_lib, border, cn):
    rng = np.random.default_rng(cn + border)
    sh, sw, dh, dw = 40, 57, 30, 70
    src = rng.integers(0, 256, (sh, sw) if cn == 1 else (sh, sw, cn), dtype=np.uint8)
    mx = (np.arange(dw, dtype=np.float32)[None, :] * 0.8 + rng.standard_normal((dh, dw)).astype(np.float32)).copy()
    my = (np.arange(dh, dtype=np.float32)[:, None] * 1.2 + rng.standard_normal((dh, dw)).astype(np.float32)).copy()
    for j, v in enumerate(REMAP_BAD + [2.0 ** 26 - 4, -2.0 ** 26]):
        mx[j, 3 * j] = v
        my[j + 2, 3 * j + 1] = v
        mx[(j + 5) % dh, 3 * j + 2] = my[(j + 5) % dh, 3 * j + 2] = v
        mx[0, dw - 1 - j] = v              # the edge columns and rows of the destination too
        my[dh - 1, j] = v
    cval = 9 if border == 0 else 0
    got = nsof_lib.remap(src, mx, my, nsof_lib.INTER_LINEAR, borderMode=border, borderValue=cval)
    assert np.array_equal(got, oracle.remap_linear(src, mx, my, border, cval))


def test_predict_region_nonfinite_flows(oracle, nsof_lib):
    rng = np.random.default_rng(6)
    h, w = 90, 120
    frame = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    flow = (rng.standard_normal((h, w, 2)) * 3).astype(np.float32)
    flow[10:20, 10:30] = _flows(10, 20)
    flow[0, :len(REMAP_BAD), 0] = REMAP_BAD
    flow[h - 1, w - len(REMAP_BAD):, 1] = REMAP_BAD
    for rect in ((0, 0, w, h), (5, 8, 60, 40)):
        x0, y0, x1, y1 = rect
        for border in (0, 1):
            got = nsof_lib.predict_region(frame, flow, rect, sign=-1, borderMode=border)
            mx, my = oracle.flow_map(flow, rect, -1)
            want = frame.copy()
            want[y0:y1, x0:x1] = oracle.remap_linear(frame, mx, my, border)
            assert np.array_equal(got, want), (rect, border)


# ---------------------------------------------------------------- 3. extreme content through every path
H, W = 64, 96
# frames in [0, s]: the oracle's flow of this pair first holds NaN at s = 3.9e20 (set A), 2.6e20 (B), 1.2e20 (C) and is
# all NaN from 4.8e20 (A), 7.0e20 (B), 3.5e20 (C) (bisected on the oracle).  The scales below give every set a finite,
# a partly NaN and an all-NaN case (A: 4e20 is 7456 of 12288 NaN).
NAN_SCALES = (1e20, 1.5e20, 2e20, 3e20, 4e20, 5e20, 1e21)
NAN_FROM = {"A": 3.9e20, "B": 2.6e20, "C": 1.2e20}


def _content():
    rng = np.random.default_rng(7)
    yy, xx = np.mgrid[0:H, 0:W]
    cases = {
        "constant": (np.full((H, W), 77, np.uint8), np.full((H, W), 77, np.uint8)),
        "constant_pair_differs": (np.full((H, W), 10, np.uint8), np.full((H, W), 250, np.uint8)),
        "checker": ((((yy // 4 + xx // 4) % 2) * 255).astype(np.uint8),
                    ((((yy + 1) // 4 + (xx + 2) // 4) % 2) * 255).astype(np.uint8)),
        "step": (np.where(xx < W // 2, 0, 255).astype(np.uint8), np.where(xx < W // 2 + 3, 0, 255).astype(np.uint8)),
        "noise_u8": (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)),
        "noise_u16": (rng.integers(0, 65536, (H, W), dtype=np.uint16), rng.integers(0, 65536, (H, W), dtype=np.uint16)),
        "negative_f32": tuple(f - np.float32(5000.0) for f in shifted_pair(8, H, W, 0.0, 900.0)),
        "large_motion": translated_pair(9, H, W, 11, -9),
    }
    for s in NAN_SCALES:
        cases[f"scale_{s:g}"] = shifted_pair(3, H, W, 0.0, s)
    return cases


CONTENT = _content()


def _want(oracle, prev, nxt, args):
    if prev.dtype == np.uint8:
        return oracle.farneback(prev, nxt, *args)
    return farneback_f32(oracle, prev.astype(np.float32), nxt.astype(np.float32), *args)


def _paths(nsof_lib, ctx, torch_dev, prev, nxt, args):
    """{path: flow} of one pair through every dispatch path the pair can take."""
    import torch
    from nsof import _lib
    from nsof.farneback import (farneback_pairs, farneback_pairs_dev, farneback_pairs_f32_dev,
                                farneback_roi_sequence_dev, farneback_roi_sequence_f32_dev)
    out = {"lone": nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, *args, ctx=ctx)}
    out["host_list"] = farneback_pairs([(prev, nxt)], dict(zip(ARGS, args)), ctx=ctx)[0]
    saved = ctx.get_option(_lib.OPT_SMALL_BATCH_JOBS)
    ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, 0)
    try:
        out["iterate_x"] = nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, *args, ctx=ctx)
    finally:
        ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, saved)
    if prev.dtype in (np.uint8, np.float32):
        f32 = prev.dtype == np.float32
        frames = torch.from_numpy(np.stack([prev, nxt])).to(torch_dev)
        flows = torch.empty((1, H, W, 2), dtype=torch.float32, device=torch_dev)
        (farneback_pairs_f32_dev if f32 else farneback_pairs_dev)([(frames[0], frames[1])], [flows[0]],
                                                                 dict(zip(ARGS, args)), ctx=ctx)
        ctx.synchronize()
        out["work_list"] = flows.cpu().numpy()[0]
        counts = torch.tensor([1, 0], dtype=torch.int32, device=torch_dev)
        rects = torch.tensor([[[0, 0, W, H]], [[0, 0, 0, 0]]], dtype=torch.int32, device=torch_dev)
        seq = torch.empty((1, H, W, 2), dtype=torch.float32, device=torch_dev)
        (farneback_roi_sequence_f32_dev if f32 else farneback_roi_sequence_dev)(frames, counts, rects, seq,
                                                                               dict(zip(ARGS, args)), ctx=ctx)
        ctx.synchronize()
        out["roi_sequence"] = seq.cpu().numpy()[0]
    return out


@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("case", list(CONTENT))
def test_extreme_content_every_path(nsof_lib, ctx, oracle, torch_dev, case, name):
    prev, nxt = CONTENT[case]
    p = PARAM_SETS[name]
    for label, args in (("", _args(p)), ("winsize 17 (unfused) ", _args(p, winsize=17))):
        want = _want(oracle, prev, nxt, args)
        for path, got in _paths(nsof_lib, ctx, torch_dev, prev, nxt, args).items():
            assert _bits_equal(got, want), (f"{label}{path}: {int((got != want).sum())} differ, NaN device "
                                            f"{int(np.isnan(got).sum())} / oracle {int(np.isnan(want).sum())}")
    if case == "constant":
        assert not want.any()
    if case.startswith("scale_"):
        assert np.isnan(_want(oracle, prev, nxt, _args(p))).any() == (float(case[6:]) >= NAN_FROM[name])


FAST_CASES = [(c, n) for c in CONTENT for n in "ABC" if not c.startswith("scale_") or float(c[6:]) < NAN_FROM[n]]


@pytest.mark.parametrize("case,name", FAST_CASES, ids=[f"{c}-{n}" for c, n in FAST_CASES])
def test_extreme_content_fast_mode(nsof_lib, ctx, oracle, case, name):
    """Every content whose oracle flow is finite (float frames up to just below each set's NaN onset included).  Past
    the onset the fast mode's own summation order decides which window sums reach inf, so its NaN mask is not the
    oracle's there (measured on the 3e20 frames with set B) and no tolerance can be stated."""
    from nsof import _lib
    prev, nxt = CONTENT[case]
    args = _args(PARAM_SETS[name])
    want = _want(oracle, prev, nxt, args)
    saved = ctx.get_option(_lib.OPT_EXACT_ROWSUMS)
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 0)
    try:
        got = nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, *args, ctx=ctx)
    finally:
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, saved)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    if (~nan).any():
        assert np.abs(got[~nan] - want[~nan]).max() <= PIPE_TOL * max(1.0, np.abs(want[~nan]).max())


# ---------------------------------------------------------------- 4. the other heads on non-finite flows
def _bad_flows(n, h, w):
    """n flows: small finite motion, a moving block, and the non-finite / huge values of part 1 at interior and border
    pixels (pair 0), the same with the whole first row NaN (pair 1), ..."""
    rng = np.random.default_rng(11)
    f = (rng.standard_normal((n, h, w, 2)) * 0.4).astype(np.float32)
    f[:, h // 4:h // 2, w // 4:w // 2] += np.float32(3.0)
    for k in range(n):
        bad = _flows(h, w)
        sel = ~np.isfinite(bad) | (np.abs(bad) > 1e9)
        f[k][sel] = bad[sel]
    f[1, 0, :, 0] = np.nan
    return f


def test_motion_mask_nonfinite_flows(nsof_lib, oracle, ctx, torch_dev):
    import torch
    from nsof import segment
    h, w = 48, 70
    flows = _bad_flows(3, h, w)
    want = [oracle.motion_mask(flows[k], 1.0, 10, 5) for k in range(3)]
    want0 = [oracle.motion_mask(flows[k], 1.0, 3, 0) for k in range(3)]   # the threshold alone, no morphology
    nan_px = np.isnan(flows[0]).any(-1)
    inf_px = np.isinf(flows[0]).any(-1) & ~nan_px
    assert not want0[0][nan_px].any() and want0[0][inf_px].all()
    for k in range(3):
        assert np.array_equal(segment.motion_mask(flows[k], ctx=ctx), want[k]), k
        assert np.array_equal(segment.motion_mask(flows[k], 1, 3, 0, ctx=ctx), want0[k]), k
    d_flows = torch.from_numpy(flows).to(torch_dev)
    d_mask = torch.empty((h, w), dtype=torch.uint8, device=torch_dev)
    torch.cuda.synchronize()
    segment.motion_mask_dev(d_flows[0], d_mask, h, w, ctx=ctx)
    ctx.synchronize()
    assert np.array_equal(d_mask.cpu().numpy(), want[0])
    got = segment.motion_mask_sequence_dev(d_flows, ctx=ctx)
    ctx.synchronize()
    for k in range(3):
        assert np.array_equal(got[k].cpu().numpy(), want[k]), k
    boxes = [[(3, 2, 40, 30)], [(0, 0, w, h)], [(10, 5, 70, 48), (0, 0, 20, 20)]]
    got = segment.motion_mask_sequence_dev(d_flows, boxes, ctx=ctx)
    ctx.synchronize()   # asynchronous on the context's stream
    got = got.cpu().numpy()
    for k in range(3):
        exp = np.zeros((h, w), np.uint8)
        for (x0, y0, x1, y1) in boxes[k]:
            exp[y0:y1, x0:x1] = oracle.motion_mask(np.ascontiguousarray(flows[k, y0:y1, x0:x1]), 1.0, 10, 5)
        assert np.array_equal(got[k], exp), k


def _colour_definition(flow, max_flow=None):
    """flow_to_image_dev's colours for a flow with NaN / inf components (its docstring): NumPy's coding of the pixels
    whose normalised u, v are not NaN, with the divisor taken over the non-NaN magnitudes; (0, 0, 0) elsewhere."""
    with np.errstate(invalid="ignore", over="ignore"):   # inf / inf and inf * 0 are the point here
        return _colour_definition_body(flow, max_flow)


def _colour_definition_body(flow, max_flow):
    from test_flowviz_cpu import cr_flow_to_image
    u, v = flow[..., 0], flow[..., 1]
    mag = np.sqrt(np.square(u) + np.square(v))
    if max_flow is None:
        top = mag[~np.isnan(mag)].max(initial=np.float32(0))
        d = np.float32(top + np.float32(1e-5))
    else:
        d = np.float32(float(max_flow) + 1e-5)
    black = np.isnan(u / d) | np.isnan(v / d)
    clean = np.where(black[..., None], np.float32(0), flow).astype(np.float32)
    img = cr_flow_to_image(clean, max_flow=None if max_flow is None and np.isfinite(d) else
                           (np.inf if max_flow is None else max_flow))
    if max_flow is None and np.isfinite(d):
        # the clean flow's own largest magnitude is the divisor's: the black pixels were NaN there
        assert np.float32(np.max(np.sqrt(np.square(clean[..., 0]) + np.square(clean[..., 1]))) + np.float32(1e-5)) == d
    img[black] = 0
    return img, black


def test_flow_to_image_nonfinite_flows(nsof_lib, ctx, torch_dev):
    from nsof import flowviz
    h, w = 40, 66
    flows = _bad_flows(3, h, w)
    finite_huge = flows[0].copy()
    finite_huge[~np.isfinite(finite_huge)] = np.float32(0.5)          # only the +-1e10 values left
    nan_only = flows[0].copy()
    nan_only[np.isinf(nan_only)] = np.float32(-2.0)
    inf_only = flows[0].copy()
    inf_only[np.isnan(inf_only)] = np.float32(0.25)
    cases = {"mixed": flows[0], "nan_row": flows[1], "huge": finite_huge, "nan_only": nan_only, "inf_only": inf_only,
             "all_nan": np.full((h, w, 2), np.nan, np.float32)}
    for name, f in cases.items():
        for mf in (None, 2.0):
            want, black = _colour_definition(f, mf)
            got = flowviz.flow_to_image_dev(_dev(torch_dev, f), max_flow=mf, ctx=ctx)
            ctx.synchronize()
            got = got.cpu().numpy()
            assert np.array_equal(got, want), (name, mf, int((got != want).any(-1).sum()))
            assert (got[~black] != 0).any(-1).all()        # no finite flow is coloured black
    # the divisor: NaN magnitudes are skipped, an infinite one makes it +inf
    import torch
    norms = torch.empty(3, dtype=torch.float32, device=torch_dev)
    stack = np.stack([nan_only, inf_only, cases["all_nan"]])
    flowviz.flow_to_image_dev(_dev(torch_dev, stack), norms=norms, ctx=ctx)
    ctx.synchronize()
    n = norms.cpu().numpy()
    m = np.sqrt(np.square(nan_only[..., 0]) + np.square(nan_only[..., 1]))
    assert n[0] == np.float32(np.nanmax(m) + np.float32(1e-5)) and np.isposinf(n[1]) and n[2] == np.float32(1e-5)
