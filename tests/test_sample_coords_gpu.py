"""GPU: the sample coordinates of the matrix update (issue_row, iterate_common.h) at the places where a floor, a
fraction or an inside test can go wrong, against the oracle bit for bit and route against route.

issue_row takes the sample's cell as floorf(x + dx) in float, decides `inside` on that float and converts to an integer
only for the clamped gather address; the oracle (and the device before) takes cvFloor's integer.  The two agree for
every float (the argument is in iterate_common.h); this file holds them to it with hand-made flow fields that put
x + dx and y + dy

  * exactly on integers, on the last valid cell (W-2, H-2) and one past it, at -1;
  * just below 0 -- in column / row 0 with |d| < 2^-25, where the fraction x + dx - floor rounds to 1.0f, and elsewhere;
  * at +-2^31 (the edge of cvFloor's range), +-3e38, +-inf and NaN,

on frames of 2x2, 1xN, Nx1, 17x9 and on a 1080p frame around its first strip boundary (columns 191-193).

Routes.  A flow field can be handed to the stage entries only, so the hand-made fields go through
  * nsof_stage_iterate in exact mode: k_iterate_x;
  * nsof_stage_update_matrices: k_update_matrices<false>, the sampling kernel of the unfused path AND of the small-batch
    form (farneback_iterate_lat.hip), then nsof_stage_blur_solve in exact mode;
  * nsof_stage_iterate in fast mode: k_iterate_q, the fast row-sum kernel, on the field of border positions only and
    within the fast mode's stage tolerance of test_farneback_gpu.py (its sums are not the oracle's running sums: no bits
    to compare, its NaNs spread differently, and next to a flow of 2^31 the tolerance would say nothing).
The stage entries refuse a fused iteration below 2x2 (as the drivers do), so 1xN and Nx1 take the second route only.
The small-batch form as a whole and the work lists (k_update_matrices<true>) take their flow from the pyramid: they
run whole pairs whose flows leave the image (a motion larger than the frame's coarsest level follows) and float pairs
whose flow is partly NaN, next to k_iterate_x on the same pairs.

Every comparison is on the bits, NaN positions included; no case is left out (the oracle's non-finite results are
compared as they are), and the oracle's flow of every finite field is checked to be finite."""
import numpy as np
import pytest

from test_extreme_content_gpu import _bits_equal
from test_farneback_gpu import _dev, _rlayout

pytestmark = pytest.mark.gpu

TINY = np.float32(2.0 ** -26)          # x = 0: 0 - TINY is just below 0 and (0 - TINY) - (-1) rounds to 1.0f
FINITE_EDGE = [np.float32(2.0 ** 31), np.float32(-2.0 ** 31), np.float32(2147483520.0), np.float32(-2147483904.0)]
NONFINITE = [np.float32(3e38), np.float32(-3e38), np.float32(np.inf), np.float32(-np.inf), np.float32(np.nan)]


def _targets(n):
    """Sample positions along an axis of n cells (as x + dx): integers, the last valid cell, one past it, -1, just
    below 0, and two ordinary fractions."""
    return [0.0, 1.0, float(n - 2), float(n - 1), float(n), -1.0, -2.0 ** -20, -0.5, n - 2 + 0.25, n - 1.5]


def _fields(h, w, cols=None):
    """(near, edge, non-finite) flow fields of one h x w frame: the positions around the frame's borders; those plus
    +-2^31; +-3e38, +-inf and NaN.  The specials sit at the pixels of `cols` (default: spread over the frame) x a few rows,
    in x, in y and in both.  A non-finite flow makes the pixel's M[3], M[4] NaN, and the oracle's running sums carry a NaN
    to every row below and every column to the right: the non-finite specials sit in the last two rows, so that the
    NaN mask that is compared is not the whole frame wherever the window leaves room."""
    rng = np.random.default_rng(h * 131 + w)
    base = (rng.standard_normal((h, w, 2)) * 0.6).astype(np.float32)
    xs = list(cols) if cols is not None else sorted({0, min(1, w - 1), w // 2, max(w - 2, 0), w - 1})
    ys = sorted({0, min(1, h - 1), h // 2, max(h - 2, 0), h - 1})
    spots = [(y, x) for y in ys for x in xs]
    fin, non = base.copy(), base.copy()
    low = [(y, x) for y in sorted({max(h - 2, 0), h - 1}) for x in xs]
    tx, ty = _targets(w), _targets(h)
    for k, (y, x) in enumerate(spots):
        vx = np.float32(tx[k % len(tx)]) - np.float32(x)      # x + vx == the target exactly (small integers, halves)
        vy = np.float32(ty[(k // 2) % len(ty)]) - np.float32(y)
        mode = k % 3
        if mode != 1:
            fin[y, x, 0] = vx
        if mode != 0:
            fin[y, x, 1] = vy
    # column / row 0: the fraction that rounds to 1.0f
    fin[ys[len(ys) // 2], 0, 0] = -TINY
    fin[0, xs[len(xs) // 2], 1] = -TINY
    fin[0, 0] = (-TINY, -TINY)
    assert np.float32(0) + fin[0, 0, 0] < 0 and (np.float32(0) + fin[0, 0, 0]) - np.float32(-1) == np.float32(1)
    edge = fin.copy()
    for k, v in enumerate(FINITE_EDGE):
        y, x = spots[(3 * k + 1) % len(spots)]
        edge[y, x, k % 2] = v
    for k, v in enumerate(NONFINITE * 3):
        y, x = low[k % len(low)]
        if k // len(NONFINITE) == 2:
            non[y, x] = (v, v)
        else:
            non[y, x, k // len(NONFINITE)] = v
    return fin, edge, non


def _expansions(oracle, h, w):
    rng = np.random.default_rng(w * 7 + h)
    img = (rng.random((h, w)) * 255).astype(np.float32)
    return oracle.polyexp(img, 5, 1.1), oracle.polyexp(np.roll(img, 1, axis=1) + np.float32(3), 5, 1.1)


def _stage_routes(ctx, oracle, torch_dev, R0, R1, flow, winsize, finite, fast=False):
    """One flow field through the stage routes; asserts each against the oracle and the routes against each other."""
    import torch
    from nsof import _lib
    h, w = flow.shape[:2]
    M = oracle.update_matrices(R0, R1, flow)
    want, _ = oracle.update_flow_blur(R0, R1, flow, M, winsize, False)
    if finite:
        assert np.isfinite(M).all() and np.isfinite(want).all(), "the finite field must stay finite in the oracle"
    dR = _dev(torch_dev, np.stack([_rlayout(R0), _rlayout(R1)])[None])
    dF = _dev(torch_dev, flow[None])
    lib = ctx._lib
    # the matrix update on its own (k_update_matrices<false>), then the exact blur + solve
    dM = torch.empty((1, 5, h, w), dtype=torch.float32, device=torch_dev)
    ctx.check(lib.nsof_stage_update_matrices(ctx.ptr, 1, dR.data_ptr(), dF.data_ptr(), w, h, dM.data_ptr()))
    ctx.synchronize()
    gotM = np.moveaxis(dM.cpu().numpy()[0], 0, -1)
    for c in range(5):
        assert _bits_equal(gotM[..., c], M[..., c]), f"k_update_matrices channel {c}: {(gotM[..., c] != M[..., c]).sum()} differ"
    out_u = torch.zeros((1, h, w, 2), dtype=torch.float32, device=torch_dev)
    ctx.check(lib.nsof_stage_blur_solve(ctx.ptr, 1, dM.data_ptr(), w, h, winsize, out_u.data_ptr()))
    ctx.synchronize()
    got_u = out_u.cpu().numpy()[0]
    assert _bits_equal(got_u, want), f"unfused stages: {(got_u != want).sum()} differ"
    if w < 2 or h < 2:
        return
    # k_iterate_x
    out_x = torch.zeros((1, h, w, 2), dtype=torch.float32, device=torch_dev)
    ctx.check(lib.nsof_stage_iterate(ctx.ptr, 1, dR.data_ptr(), dF.data_ptr(), w, h, winsize, out_x.data_ptr()))
    ctx.synchronize()
    got_x = out_x.cpu().numpy()[0]
    assert _bits_equal(got_x, want), f"k_iterate_x: {(got_x != want).sum()} differ"
    assert _bits_equal(got_x, got_u)
    if not fast:
        return
    # k_iterate_q (fast mode): test_farneback_gpu.py's stage tolerance
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 0)
    try:
        out_q = torch.zeros((1, h, w, 2), dtype=torch.float32, device=torch_dev)
        ctx.check(lib.nsof_stage_iterate(ctx.ptr, 1, dR.data_ptr(), dF.data_ptr(), w, h, winsize, out_q.data_ptr()))
        ctx.synchronize()
    finally:
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 1)
    got_q = out_q.cpu().numpy()[0]
    d = np.abs(got_q - want)
    assert d.max() <= 1e-6 * max(1.0, np.abs(want).max()), d.max()
    if want.size >= 10000:                 # "under 1 % of the values differ" says nothing on a frame of 8 or 300 values
        assert (got_q != want).mean() < 0.01


@pytest.mark.parametrize("shape", [(2, 2), (1, 23), (23, 1), (9, 17), (17, 9)])
@pytest.mark.parametrize("winsize", [3, 15])
def test_hand_made_flows_small_frames(ctx, oracle, torch_dev, shape, winsize):
    h, w = shape
    R0, R1 = _expansions(oracle, h, w)
    near, edge, non = _fields(h, w)
    _stage_routes(ctx, oracle, torch_dev, R0, R1, near, winsize, True, fast=True)
    _stage_routes(ctx, oracle, torch_dev, R0, R1, edge, winsize, True)
    _stage_routes(ctx, oracle, torch_dev, R0, R1, non, winsize, False)


def test_hand_made_flows_at_1080p_strip_boundary(ctx, oracle, torch_dev):
    """Columns 191-193: the last column of k_iterate_x's first strip, the first two of its second (and their halo
    columns in the neighbour's ring)."""
    h, w = 1080, 1920
    R0, R1 = _expansions(oracle, h, w)
    near, edge, non = _fields(h, w, cols=(191, 192, 193))
    _stage_routes(ctx, oracle, torch_dev, R0, R1, near, 15, True, fast=True)
    _stage_routes(ctx, oracle, torch_dev, R0, R1, edge, 15, True)
    _stage_routes(ctx, oracle, torch_dev, R0, R1, non, 15, False)


def _pipeline_routes(nsof_lib, ctx, torch_dev, prev, nxt, args):
    import torch
    from nsof import _lib
    from nsof.farneback import farneback_pairs, farneback_pairs_dev, farneback_pairs_f32_dev
    names = ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags")
    h, w = prev.shape
    out = {"small_batch": nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, *args, ctx=ctx)}
    ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, 0)
    try:
        out["iterate_x"] = nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, *args, ctx=ctx)
    finally:
        ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, 64)
    out["host_list"] = farneback_pairs([(prev, nxt)], dict(zip(names, args)), ctx=ctx)[0]
    frames = torch.from_numpy(np.stack([prev, nxt])).to(torch_dev)
    flows = torch.empty((1, h, w, 2), dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    (farneback_pairs_f32_dev if prev.dtype == np.float32 else farneback_pairs_dev)(
        [(frames[0], frames[1])], [flows[0]], dict(zip(names, args)), ctx=ctx)
    ctx.synchronize()
    out["work_list"] = flows.cpu().numpy()[0]
    return out


@pytest.mark.parametrize("args", [(0.5, 3, 15, 3, 5, 1.2, 0), (0.6, 3, 3, 3, 10, 1.05, 0), (0.6, 3, 4, 2, 1, 1.05, 0)],
                         ids=["A", "B", "C"])
def test_small_batch_and_work_list_samples_leave_the_image(nsof_lib, ctx, oracle, torch_dev, args):
    """Whole pairs through the small-batch form, k_iterate_x and the work lists: a translation of (11, -9) px on 64x96
    (the flow's samples leave the frame along two borders) and float frames scaled to where the flow is partly NaN."""
    from test_farneback_f64 import translated_pair
    from test_float_reference import farneback_f32, shifted_pair
    prev, nxt = translated_pair(9, 64, 96, 11, -9)
    want = oracle.farneback(prev, nxt, *args)
    assert np.abs(want).max() > 2.0          # the samples do move
    for path, got in _pipeline_routes(nsof_lib, ctx, torch_dev, prev, nxt, args).items():
        assert _bits_equal(got, want), (path, int((got != want).sum()))
    fp, fn = shifted_pair(3, 64, 96, 0.0, 4e20)
    fp, fn = fp.astype(np.float32), fn.astype(np.float32)
    want = farneback_f32(oracle, fp, fn, *args)
    assert np.isnan(want).any()
    for path, got in _pipeline_routes(nsof_lib, ctx, torch_dev, fp, fn, args).items():
        assert _bits_equal(got, want), (path, int(np.isnan(got).sum()), int(np.isnan(want).sum()))
