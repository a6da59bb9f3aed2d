"""OPTFLOW_FARNEBACK_GAUSSIAN (flags = 256) on every Farneback entry: k_update_matrices + k_gauss_blur_solve per iteration.

The GPU equals the float32 restatement of tests/farneback_gauss.py BIT FOR BIT: at stage level over the tile seams of the
LDS kernel, windows wider than the image, both kernel forms and up to window 65; through the lone call, the device batch,
the device sequence, host and device work lists and the gated ROI sequence; on 16-bit and float frames.  The launch
counters show the route, and flags the library does not build stay refused with the output untouched.
"""
import numpy as np
import pytest

import farneback_gauss as G
from test_exact_paths_gpu import _batch_and_sequence, _diff, _frames
from test_farneback_gpu import _dev, _level_state, _planar
from test_winsize_routes_gpu import _counted, _crops, _list_shapes

pytestmark = pytest.mark.gpu

ITERATIONS = 2
LDS_MAX_M = 16   # NSOF_GAUSS_LDS_MAX_M in csrc/nsof_internal.h: larger half-widths take k_gauss_blur_solve_general
STAGE_WINDOWS = [2, 3, 4, 5, 14, 15, 16, 17, 32, 2 * LDS_MAX_M + 1, 2 * LDS_MAX_M + 2, 65]
CALL_WINDOWS = [3, 15, 33]


def _gauss_tile():
    """(columns, rows) of outputs a k_gauss_blur_solve workgroup owns: GS_TX, GS_TY in csrc/farneback_gauss.hip."""
    return 64, 32


def _params(winsize, flags=G.GAUSSIAN):
    return (0.5, 2, winsize, ITERATIONS, 5, 1.1, flags)


def _want(prev, nxt, params):
    """The reference flow of one pair; a frame of at least 33 px on both sides must give a finite field that moves by more
    than a pixel somewhere."""
    prev, nxt = np.ascontiguousarray(prev), np.ascontiguousarray(nxt)
    want = G.farneback_gauss(prev, nxt, *params)
    if min(prev.shape) >= 33 and params[3] > 0:
        assert np.isfinite(want).all() and np.abs(want).max() > 1.0, (prev.shape, params, float(np.abs(want).max()))
    return want


# ---- 1. the stage -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def matrices(oracle):
    """(h, w) -> the matrices M [h][w][5] of two different synthetic pairs, made once per shape and shared read-only."""
    cache = {}

    def get(h, w):
        if (h, w) not in cache:
            out = []
            for seed in (h * 1000 + w, h * 1000 + w + 500):
                fr = _frames(seed, 2, h, w)
                R0, R1, flow = _level_state(oracle, fr[0], fr[1], 5, 1.1, seed % 97)
                M = oracle.update_matrices(R0, R1, flow)
                M.setflags(write=False)
                out.append(M)
            assert not np.array_equal(out[0], out[1])
            cache[(h, w)] = out
        return cache[(h, w)]
    return get


def _stage_shapes(m):
    tx, ty = _gauss_tile()
    return [(1, 1), (1, 9), (9, 1), (2, 2),                      # a window wider than the image on one or both axes
            (5, tx - 1), (5, tx), (5, tx + 1),                   # the right edge before, on and past a tile seam
            (ty + 1, 2 * tx + 1),                                # a partial last tile on both axes, three tiles across
            (2 * m + 6, m + 1)]                                  # a window and a half of rows, a column past the halo


@pytest.mark.parametrize("winsize", STAGE_WINDOWS)
def test_stage_gauss_blur_solve(ctx, torch_dev, matrices, winsize):
    """nsof_stage_gauss_blur_solve on a launch of three pairs -- A, B, A: two different pairs, and one pair twice -- against
    gauss_blur_solve.  Windows up to 33 run the LDS kernel, 34 and 65 the general one; 2m and 2m + 1 share their taps."""
    import torch
    m = winsize // 2
    for h, w in _stage_shapes(m):
        A, B = matrices(h, w)
        want = [G.gauss_blur_solve(M, winsize) for M in (A, B)]
        assert all(np.isfinite(x).all() for x in want) and want[0].any(), (winsize, (h, w))
        dM = _dev(torch_dev, np.stack([_planar(A), _planar(B), _planar(A)]))
        out = torch.full((3, h, w, 2), 7.0, dtype=torch.float32, device=torch_dev)
        torch.cuda.synchronize()
        ctx.check(ctx._lib.nsof_stage_gauss_blur_solve(ctx.ptr, 3, dM.data_ptr(), w, h, winsize, out.data_ptr()))
        ctx.synchronize()
        got = out.cpu().numpy()
        for i, wt in enumerate((want[0], want[1], want[0])):
            assert np.array_equal(got[i], wt), (winsize, (h, w), i, _diff(got[i], wt))


def test_stage_refuses_bad_arguments(ctx, torch_dev):
    import torch
    from nsof import _lib
    dM = torch.zeros((1, 5, 4, 4), dtype=torch.float32, device=torch_dev)
    out = torch.full((1, 4, 4, 2), 7.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    stage = ctx._lib.nsof_stage_gauss_blur_solve
    assert stage(ctx.ptr, 1, dM.data_ptr(), 4, 4, 1, out.data_ptr()) == _lib.NSOF_EINVAL
    assert stage(ctx.ptr, 0, dM.data_ptr(), 4, 4, 3, out.data_ptr()) == _lib.NSOF_EINVAL
    assert stage(ctx.ptr, 1, dM.data_ptr(), 4, 4, 196, out.data_ptr()) == _lib.NSOF_EUNSUPPORTED
    ctx.synchronize()
    assert (out == 7.0).all()


# ---- 2. whole calls -----------------------------------------------------------------------------------------------------
def _check_all(nsof_lib, ctx, frames, params, tag):
    want = [_want(frames[i], frames[i + 1], params) for i in range(frames.shape[0] - 1)]
    got_b, got_s = _batch_and_sequence(nsof_lib, ctx, frames, params)
    for i, wt in enumerate(want):
        assert np.array_equal(got_b[i], wt), (tag, "batch", i, _diff(got_b[i], wt))
        assert np.array_equal(got_s[i], wt), (tag, "sequence", i, _diff(got_s[i], wt))
    one = nsof_lib.calcOpticalFlowFarneback(frames[0], frames[1], None, *params, ctx=ctx)
    assert np.array_equal(one, want[0]), (tag, "lone call", _diff(one, want[0]))


@pytest.mark.parametrize("winsize", CALL_WINDOWS)
def test_lone_batch_and_sequence(nsof_lib, ctx, winsize):
    """Three pairs of 45 x 200 through the lone call, farneback_batch and farneback_sequence."""
    _check_all(nsof_lib, ctx, _frames(45 * 1000 + 200, 4, 45, 200), _params(winsize), winsize)


@pytest.mark.parametrize("winsize", CALL_WINDOWS)
def test_three_levels(nsof_lib, ctx, winsize):
    params = (0.5, 3, winsize, ITERATIONS, 5, 1.1, G.GAUSSIAN)
    assert nsof_lib.effective_levels(257, 130, 0.5, 3) + 1 == 3
    _check_all(nsof_lib, ctx, _frames(130 * 1000 + 257, 2, 130, 257), params, winsize)


@pytest.mark.parametrize("winsize", CALL_WINDOWS)
def test_generic_pyramid_scale(nsof_lib, ctx, winsize):
    params = (0.6, 3, winsize, ITERATIONS, 7, 1.5, G.GAUSSIAN)
    _check_all(nsof_lib, ctx, _frames(97 * 1000 + 131, 2, 97, 131), params, winsize)


@pytest.mark.parametrize("winsize", CALL_WINDOWS)
def test_16_bit_and_float_frames(nsof_lib, ctx, winsize):
    """Only the pyramid reads the frames: uint16 and float32 frames holding the 8-bit values give the same flow."""
    fr = _frames(70 * 1000 + 33, 2, 70, 33)
    params = _params(winsize)
    want = _want(fr[0], fr[1], params)
    for dtype in (np.float32, np.uint16):
        got = nsof_lib.calcOpticalFlowFarneback(fr[0].astype(dtype), fr[1].astype(dtype), None, *params, ctx=ctx)
        assert np.array_equal(got, want), (winsize, dtype, _diff(got, want))


def test_params_object_and_many(nsof_lib, ctx):
    """FarnebackParams(flags=256) and farneback_many pass the flag on."""
    fr = _frames(45 * 1000 + 200, 3, 45, 200)
    P = nsof_lib.FarnebackParams(0.5, 2, 15, ITERATIONS, 5, 1.1, nsof_lib.OPTFLOW_FARNEBACK_GAUSSIAN)
    want = [_want(fr[i], fr[i + 1], _params(15)) for i in range(2)]
    one = nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, **P.as_kwargs(), ctx=ctx)
    assert np.array_equal(one, want[0])
    many = nsof_lib.farneback_many([(fr[0], fr[1]), (fr[1], fr[2])], P, n_streams=2)
    for got, wt in zip(many, want):
        assert np.array_equal(got, wt), _diff(got, wt)


# ---- 3. work lists -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("winsize", CALL_WINDOWS)
def test_work_lists(nsof_lib, ctx, torch_dev, winsize):
    """farneback_pairs and farneback_pairs_dev on crops of six shapes (non-contiguous views, the 2 x 2 item among them):
    each flow equals the lone call and the reference.  Every item runs on its own: (L_i + 1) I blur and matrix scopes per
    item, none of the fused iteration."""
    import torch
    from nsof import _lib
    m = winsize // 2
    params = _params(winsize)
    P = nsof_lib.FarnebackParams(*params)
    shapes = _list_shapes("S", m)
    assert (2, 2) in shapes
    pairs = _crops(700 + winsize, shapes)
    want = [_want(a, b, params) for a, b in pairs]
    scopes = sum(nsof_lib.effective_levels(w, h, 0.5, 2) + 1 for h, w in shapes) * ITERATIONS
    flows, counts = _counted(ctx, lambda: nsof_lib.farneback_pairs(pairs, P, ctx=ctx))
    assert counts == {_lib.K_ITERATE: 0, _lib.K_BLUR: scopes, _lib.K_UPDMAT: scopes}, (winsize, counts)
    for i, ((a, b), f, wt) in enumerate(zip(pairs, flows, want)):
        assert np.array_equal(f, wt), (winsize, "host list", shapes[i], _diff(f, wt))
        one = nsof_lib.calcOpticalFlowFarneback(a, b, None, *params, ctx=ctx)
        assert np.array_equal(one, wt), (winsize, "lone call", shapes[i], _diff(one, wt))
    # the device list: crops of frames in HBM, flows into crops of a canvas
    big_h, big_w = max(h for h, _ in shapes) + 3, max(w for _, w in shapes) + 5
    d_pairs, d_flows = [], []
    for (a, b), (h, w) in zip(pairs, shapes):
        fa = torch.zeros((big_h, big_w), dtype=torch.uint8, device=torch_dev)
        fb = torch.zeros_like(fa)
        fa[1:1 + h, 3:3 + w] = torch.from_numpy(np.ascontiguousarray(a)).to(torch_dev)
        fb[1:1 + h, 3:3 + w] = torch.from_numpy(np.ascontiguousarray(b)).to(torch_dev)
        d_pairs.append((fa[1:1 + h, 3:3 + w], fb[1:1 + h, 3:3 + w]))
        d_flows.append(torch.full((big_h, big_w, 2), 7.0, dtype=torch.float32, device=torch_dev)[2:2 + h, 1:1 + w])
    torch.cuda.synchronize()
    nsof_lib.farneback_pairs_dev(d_pairs, d_flows, P, ctx=ctx)
    ctx.synchronize()
    for i, (f, wt) in enumerate(zip(d_flows, want)):
        assert np.array_equal(f.cpu().numpy(), wt), (winsize, "device list", shapes[i], _diff(f.cpu().numpy(), wt))


@pytest.mark.parametrize("winsize", CALL_WINDOWS)
def test_uniform_work_list(nsof_lib, ctx, torch_dev, winsize):
    """A list of three equal crops at constant strides goes to the uniform driver as one batch: (L + 1) I scopes in all."""
    import torch
    from nsof import _lib
    params = _params(winsize)
    P = nsof_lib.FarnebackParams(*params)
    frames = _frames(45 * 1000 + 200, 4, 45, 200)
    want = [_want(frames[i], frames[i + 1], params) for i in range(3)]
    host = nsof_lib.farneback_pairs([(frames[i], frames[i + 1]) for i in range(3)], P, ctx=ctx)
    for i, wt in enumerate(want):
        assert np.array_equal(host[i], wt), (winsize, "host", i, _diff(host[i], wt))
    d = torch.from_numpy(frames).to(torch_dev)
    out = torch.full((3, 45, 200, 2), 7.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()

    def run():
        nsof_lib.farneback_pairs_dev([(d[i], d[i + 1]) for i in range(3)], [out[i] for i in range(3)], P, ctx=ctx)
        ctx.synchronize()
    _, counts = _counted(ctx, run)
    scopes = (nsof_lib.effective_levels(200, 45, 0.5, 2) + 1) * ITERATIONS
    assert counts == {_lib.K_ITERATE: 0, _lib.K_BLUR: scopes, _lib.K_UPDMAT: scopes}, (winsize, counts)
    got = out.cpu().numpy()
    for i, wt in enumerate(want):
        assert np.array_equal(got[i], wt), (winsize, "device", i, _diff(got[i], wt))


def test_roi_sequence(nsof_lib, ctx, torch_dev):
    """farneback_roi_sequence_dev on 3 frames of 96 x 128 with two overlapping rectangles per frame == the crops' reference
    flows pasted on the host in table order."""
    import torch
    H, W = 96, 128
    frames = _frames(96 * 1000 + 128, 3, H, W)
    table = [(8, 10, 88, 70), (60, 40, 124, 90)]   # x0, y0, x1, y1
    params = _params(15)
    rects = np.zeros((3, 2, 4), np.int32)
    rects[:] = table
    counts = np.full(3, 2, np.int32)
    want = np.zeros((2, H, W, 2), np.float32)
    for k in range(2):
        for x0, y0, x1, y1 in table:
            want[k, y0:y1, x0:x1] = _want(frames[k, y0:y1, x0:x1], frames[k + 1, y0:y1, x0:x1], params)
    d_frames, d_counts, d_rects = (torch.from_numpy(a).to(torch_dev) for a in (frames, counts, rects))
    flows = torch.full((2, H, W, 2), 7.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    n_calls, _ = nsof_lib.farneback_roi_sequence_dev(d_frames, d_counts, d_rects, flows, nsof_lib.FarnebackParams(*params),
                                                      gate_frame=0, ctx=ctx)
    ctx.synchronize()
    assert n_calls == 4
    got = flows.cpu().numpy()
    assert np.array_equal(got, want), _diff(got, want)


# ---- 4. the route ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("winsize", CALL_WINDOWS)
def test_route_counts(nsof_lib, ctx, oracle, winsize):
    """A Gaussian call opens (L + 1) I K_BLUR and K_UPDMAT scopes and no K_ITERATE scope, whatever the window; the same
    context with flags = 0 keeps its routes: the small-batch form (2 (L + 1) I K_ITERATE scopes) for window 3 and 15, the
    unfused exact pair for 33."""
    from nsof import _lib
    fr = _frames(45 * 1000 + 200, 2, 45, 200)
    scopes = (nsof_lib.effective_levels(200, 45, 0.5, 2) + 1) * ITERATIONS
    got, counts = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, *_params(winsize), ctx=ctx))
    assert counts == {_lib.K_ITERATE: 0, _lib.K_BLUR: scopes, _lib.K_UPDMAT: scopes}, (winsize, counts)
    assert np.array_equal(got, _want(fr[0], fr[1], _params(winsize)))
    box, counts = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, *_params(winsize, 0), ctx=ctx))
    if winsize <= 15:
        assert counts == {_lib.K_ITERATE: 2 * scopes, _lib.K_BLUR: 0, _lib.K_UPDMAT: 0}, (winsize, counts)
    else:
        assert counts == {_lib.K_ITERATE: 0, _lib.K_BLUR: scopes, _lib.K_UPDMAT: scopes}, (winsize, counts)
    assert np.array_equal(box, oracle.farneback(fr[0], fr[1], *_params(winsize, 0)))


def test_no_leak_between_forms(nsof_lib, ctx, oracle):
    """One context runs flags 256, 0 and 256: the middle flow is the box oracle's, the outer two the Gaussian reference."""
    fr = _frames(45 * 1000 + 200, 2, 45, 200)
    want_g = _want(fr[0], fr[1], _params(15))
    want_b = oracle.farneback(fr[0], fr[1], *_params(15, 0))
    assert not np.array_equal(want_g, want_b)
    for flags, wt in ((G.GAUSSIAN, want_g), (0, want_b), (G.GAUSSIAN, want_g)):
        got = nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, *_params(15, flags), ctx=ctx)
        assert np.array_equal(got, wt), (flags, _diff(got, wt))


# ---- 5. what stays refused -----------------------------------------------------------------------------------------------
def _refused(nsof_lib, call):
    from nsof import _lib
    with pytest.raises(nsof_lib.error) as e:
        call()
    assert e.value.status == _lib.NSOF_EUNSUPPORTED, str(e.value)
    return str(e.value)


@pytest.mark.parametrize("flags,winsize", [(4, 15), (260, 15), (1, 15), (256, 1)])
def test_refusals(nsof_lib, ctx, torch_dev, flags, winsize):
    """OPTFLOW_USE_INITIAL_FLOW alone or with the Gaussian flag, an unknown bit, and winsize 1 with the Gaussian flag: refused
    on the lone, batch and list entries before anything runs, the output untouched."""
    import torch
    fr = _frames(45 * 1000 + 200, 2, 45, 200)
    params = (0.5, 2, winsize, ITERATIONS, 5, 1.1, flags)
    P = nsof_lib.FarnebackParams(*params)
    out = np.full((45, 200, 2), 7.0, np.float32)
    msg = _refused(nsof_lib, lambda: nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], out, *params, ctx=ctx))
    if flags != 256:
        assert "OPTFLOW_USE_INITIAL_FLOW" in msg
    assert (out == 7.0).all()
    d = torch.from_numpy(fr).to(torch_dev)
    d_out = torch.full((1, 45, 200, 2), 7.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    _refused(nsof_lib, lambda: nsof_lib.farneback_batch(d[:1], d[1:], d_out, 1, 45, 200, P, ctx=ctx))
    _refused(nsof_lib, lambda: nsof_lib.farneback_pairs([(fr[0], fr[1])], P, [out], ctx=ctx))
    _refused(nsof_lib, lambda: nsof_lib.farneback_pairs_dev([(d[0], d[1])], [d_out[0]], P, ctx=ctx))
    ctx.synchronize()
    assert (out == 7.0).all() and bool((d_out == 7.0).all())


def test_zero_iterations(nsof_lib, ctx):
    """iterations = 0 with the flag: the upsampled zero field, as the reference gives it."""
    fr = _frames(45 * 1000 + 200, 2, 45, 200)
    params = (0.5, 2, 15, 0, 5, 1.1, G.GAUSSIAN)
    want = G.farneback_gauss(fr[0], fr[1], *params)
    assert want.shape == (45, 200, 2) and not want.any()
    got = nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], np.full((45, 200, 2), 7.0, np.float32), *params, ctx=ctx)
    assert np.array_equal(got, want)
