"""GPU: the nsof_stage_* entry points against the float64 reference (tests/farneback_f64.py) and, bit for bit, against the
oracle, at the edge shapes of tests/test_farneback_f64.py: 1x1, one row, one column, frames smaller than the expansion's
neighbourhood, the pyramid kernel and the blur window; every poly_n, every window, pyr_scale 0.3 .. 0.8.  Exact mode
(the default) throughout: every stage here has an oracle twin with the same operation order."""
import numpy as np
import pytest

import farneback_f64 as F
from test_farneback_f64 import SCALES, SHAPES, _check, _ids, _noise, _stage_inputs
from test_farneback_gpu import _dev, _planar, _rlayout

pytestmark = pytest.mark.gpu

EDGE = SHAPES + [(2, 2), (31, 45)]


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got.view(np.int32), np.ascontiguousarray(want, np.float32).view(np.int32)), \
        f"{what}: {(got != want).sum()} values differ from the oracle"


@pytest.mark.parametrize("shape", EDGE, ids=_ids(EDGE))
def test_polyexp_stage(ctx, oracle, torch_dev, shape):
    import torch
    h, w = shape
    img = _noise(h * 7 + w, shape)
    d = _dev(torch_dev, img)
    out = torch.empty(5 * h * w, dtype=torch.float32, device=torch_dev)
    for n in range(1, 11):
        for sigma in (0.0, 1.2, 0.3 * n + 0.7):
            ctx.check(ctx._lib.nsof_stage_polyexp(ctx.ptr, 1, d.data_ptr(), w, h, n, sigma, out.data_ptr()))
            ctx.synchronize()
            got = out.cpu().numpy()
            want = oracle.polyexp(img, n, sigma)
            _same(got, _rlayout(want), f"polyexp n={n} sigma={sigma}")
            ref, tol = F.polyexp(img, n, sigma)
            _check(got[:4 * h * w].reshape(h, w, 4), (ref[..., :4], tol[..., :4]), f"polyexp n={n} ch0-3")
            _check(got[4 * h * w:].reshape(h, w), (ref[..., 4], tol[..., 4]), f"polyexp n={n} ch4")


@pytest.mark.parametrize("shape", SHAPES + [(33, 47), (61, 83)], ids=_ids(SHAPES + [(33, 47), (61, 83)]))
def test_pyr_level_stages(ctx, oracle, torch_dev, shape):
    """8-bit (nsof_stage_pyr_level) and float (nsof_stage_pyr_level_f32) frames, every scale and level with a
    non-empty result and a kernel of at most 63 taps."""
    import torch
    from test_float_reference import pyr_level_f32
    h, w = shape
    u8 = np.random.default_rng(w * 31 + h).integers(0, 256, shape, dtype=np.uint8)
    f32 = _noise(w + h, shape, 1000.0) - np.float32(300.0)
    du8, df32 = _dev(torch_dev, u8), _dev(torch_dev, f32)
    for ps in SCALES:
        for k in range(0, 4):
            wk, hk, ksize, _ = F.level_geometry(w, h, ps, k)
            if wk < 1 or hk < 1 or ksize > 63:
                continue
            out = torch.empty((hk, wk), dtype=torch.float32, device=torch_dev)
            ctx.check(ctx._lib.nsof_stage_pyr_level(ctx.ptr, 1, du8.data_ptr(), w, h * w, w, h, ps, k, out.data_ptr()))
            ctx.synchronize()
            got = out.cpu().numpy()
            _same(got, oracle.pyr_level(u8, ps, k), f"pyr_level u8 ps={ps} k={k}")
            _check(got, F.pyr_level(u8, ps, k), f"pyr_level u8 ps={ps} k={k}")
            ctx.check(ctx._lib.nsof_stage_pyr_level_f32(ctx.ptr, 1, df32.data_ptr(), 4 * w, 4 * h * w, w, h, ps, k,
                                                        out.data_ptr()))
            ctx.synchronize()
            got = out.cpu().numpy()
            _same(got, pyr_level_f32(oracle, f32, ps, k), f"pyr_level f32 ps={ps} k={k}")
            _check(got, F.pyr_level(f32, ps, k), f"pyr_level f32 ps={ps} k={k}")


@pytest.mark.parametrize("shape", EDGE + [(11, 11)], ids=_ids(EDGE + [(11, 11)]))
def test_update_matrices_stage(ctx, oracle, torch_dev, shape):
    import torch
    h, w = shape
    R0, R1, flow = _stage_inputs(h * 100 + w, h, w)
    dR = _dev(torch_dev, np.stack([_rlayout(R0), _rlayout(R1)])[None])
    dF = _dev(torch_dev, flow[None])
    out = torch.empty((1, 5, h, w), dtype=torch.float32, device=torch_dev)
    ctx.check(ctx._lib.nsof_stage_update_matrices(ctx.ptr, 1, dR.data_ptr(), dF.data_ptr(), w, h, out.data_ptr()))
    ctx.synchronize()
    got = np.ascontiguousarray(np.moveaxis(out.cpu().numpy()[0], 0, -1))
    _same(got, oracle.update_matrices(R0, R1, flow), "update_matrices")
    _check(got, F.update_matrices(R0, R1, flow), "update_matrices")


@pytest.mark.parametrize("shape", EDGE, ids=_ids(EDGE))
def test_blur_solve_and_iterate_stages(ctx, oracle, torch_dev, shape):
    """blur + solve at every window 2..31; the fused iteration (update_matrices + blur + solve in one kernel) at every
    window it takes (2..15) on frames of at least 2x2."""
    import torch
    h, w = shape
    R0, R1, flow = _stage_inputs(h * 100 + w + 7, h, w)
    M = oracle.update_matrices(R0, R1, flow)
    dM = _dev(torch_dev, _planar(M)[None])
    dR = _dev(torch_dev, np.stack([_rlayout(R0), _rlayout(R1)])[None])
    dF = _dev(torch_dev, flow[None])
    out = torch.empty((1, h, w, 2), dtype=torch.float32, device=torch_dev)
    for ws in range(2, 32):
        ctx.check(ctx._lib.nsof_stage_blur_solve(ctx.ptr, 1, dM.data_ptr(), w, h, ws, out.data_ptr()))
        ctx.synchronize()
        got = out.cpu().numpy()[0]
        want, _ = oracle.update_flow_blur(R0, R1, flow, M, ws, False)
        _same(got, want, f"blur_solve winsize={ws}")
        ref = F.blur_solve(M, ws)
        _check(got, ref, f"blur_solve winsize={ws}")
        if ws <= 15 and h >= 2 and w >= 2:
            out.zero_()
            ctx.check(ctx._lib.nsof_stage_iterate(ctx.ptr, 1, dR.data_ptr(), dF.data_ptr(), w, h, ws, out.data_ptr()))
            ctx.synchronize()
            got = out.cpu().numpy()[0]
            _same(got, want, f"iterate winsize={ws}")
            _check(got, ref, f"iterate winsize={ws}")


@pytest.mark.parametrize("src,dst", [((1, 1), (2, 2)), ((1, 3), (2, 5)), ((3, 1), (5, 2)), ((2, 2), (3, 4)),
                                     ((5, 7), (9, 11)), ((9, 16), (17, 27)), ((17, 23), (57, 77)),
                                     ((20, 150), (40, 300))])
def test_flow_upsample_stage(ctx, oracle, torch_dev, src, dst):
    import torch
    f = (np.random.default_rng(src[0] * 7 + dst[1]).standard_normal(src + (2,)) * 4).astype(np.float32)
    d = _dev(torch_dev, f[None])
    out = torch.empty((1,) + dst + (2,), dtype=torch.float32, device=torch_dev)
    for ps in (0.3, 0.5, 0.6, 0.8):
        ctx.check(ctx._lib.nsof_stage_flow_upsample(ctx.ptr, 1, d.data_ptr(), src[1], src[0], out.data_ptr(), dst[1],
                                                    dst[0], ps))
        ctx.synchronize()
        got = out.cpu().numpy()[0]
        _same(got, oracle.resize_linear(f, dst[1], dst[0]) * np.float32(1.0 / ps), f"flow_upsample ps={ps}")
        _check(got, F.flow_upsample(f, dst[1], dst[0], ps), f"flow_upsample ps={ps}")


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_pipeline_known_answers(nsof_lib, ctx, name):
    """Constant frames give exactly zero flow; integer translations are recovered as on the CPU
    (tests/test_farneback_f64.py)."""
    from test_farneback_f64 import CASES, PARAMS, translated_pair
    p = PARAMS[name]
    for v in (0, 1, 128, 255):
        a = np.full((70, 90), v, np.uint8)
        assert not nsof_lib.calcOpticalFlowFarneback(a, a, None, *p, ctx=ctx).any(), v
    for n, (dx, dy) in CASES:
        if n != name:
            continue
        prev, nxt = translated_pair(21, 120, 160, dx, dy)
        flow = nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, *p, ctx=ctx)
        err = np.hypot(flow[..., 0] - dx, flow[..., 1] - dy)[24:-24, 24:-24]
        assert err.mean() < 0.01 and np.percentile(err, 95) < 0.02, (dx, dy, err.mean())
