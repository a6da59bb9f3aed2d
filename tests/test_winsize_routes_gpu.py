"""Every window size 2..15 on every route of the fused Farneback iteration.

The iteration kernels are templated on the window half-width MH = winsize / 2 (1..7) and instantiated once more per route:

  * k_iterate_x<MH, HET>                            exact order, one kernel (uniform batches / work lists);
  * k_update_matrices<HET> + k_lat_colsum<HET> + k_lat_rowscan<MH, HET, ROWS>
                                                    exact order, small-batch form, ROWS = 4 or 8 rows per workgroup;
  * k_iterate_q<MH, HET>                            fast mode, strips of QGeom<MH>::SW columns.

Each instance keeps its own ring depth, halo, row-start sums and strip seams, so each is run here at all 14 windows (both
parities of an MH differ in block_size), on the shapes where those differ: the last strip narrower than, at and past the
halo, several hand-overs, the row scan's 32-column tiles, the column sums' unclamped-load and 256-row thresholds, the
ROWS switch, and both work-list forms.  Exact mode is compared bit for bit with the CPU oracle; fast mode is held to the
rules the neighbouring tests already apply.  The launch counters show that a case ran the route it names.
"""
import numpy as np
import pytest

from test_exact_paths_gpu import _batch_and_sequence, _diff, _frames, jobs  # noqa: F401  (jobs is a fixture)
from test_farneback_gpu import PIPE_TOL, _dev, _level_state, _rlayout, fast_mode  # noqa: F401  (fast_mode is a fixture)

pytestmark = pytest.mark.gpu

WINSIZES = list(range(2, 16))
ITERATIONS = 2


def _params(winsize):
    return (0.5, 2, winsize, ITERATIONS, 5, 1.1, 0)


def _q_strip(m):
    """Columns a k_iterate_q<MH> workgroup solves: QGeom<MH>::SW in csrc/farneback_iterate.hip."""
    return (256 - 2 * m) & ~3


def _want_flow(oracle, prev, nxt, params):
    """The oracle's flow of one pair; a frame of at least 33 px on both sides must give a finite field that moves by more
    than a pixel somewhere (an all-zero or non-finite reference would let a broken kernel pass)."""
    want = oracle.farneback(prev, nxt, *params)
    if min(prev.shape) >= 33:
        assert np.isfinite(want).all() and np.abs(want).max() > 1.0, (prev.shape, params, float(np.abs(want).max()))
    return want


def _counted(ctx, call):
    """Runs `call` with the iteration, blur and matrix-update scopes counted -> (its result, {kernel id: scopes})."""
    from nsof import _lib
    ids = (_lib.K_ITERATE, _lib.K_BLUR, _lib.K_UPDMAT)
    ctx.prof_enable(*ids)
    try:
        for k in ids:
            ctx.prof_collect(k)   # start from zero
        out = call()
        return out, {k: ctx.prof_collect(k)[1] for k in ids}
    finally:
        ctx.prof_enable()


def _assert_uniform_route(nsof_lib, counts, form, shape, winsize, calls, tag):
    """A uniform call of L + 1 pyramid levels and I iterations opens (L + 1) I K_ITERATE scopes in the one-kernel form
    (nsof_launch_iterate_x) and 2 (L + 1) I in the small-batch form (one in nsof_launch_iterate_lat around the matrix and
    column-sum kernels, one in launch_lat_rowscan); neither opens a K_BLUR or K_UPDMAT scope (the unfused pair)."""
    from nsof import _lib
    h, w = shape
    levels = nsof_lib.effective_levels(w, h, 0.5, 2) + 1
    per_call = {"one_kernel": 1, "small_batch": 2}[form] * levels * ITERATIONS
    assert counts[_lib.K_ITERATE] == calls * per_call, (tag, winsize, shape, form, counts)
    assert counts[_lib.K_BLUR] == 0 and counts[_lib.K_UPDMAT] == 0, (tag, winsize, shape, form, counts)


# ---- 1. stage level: the seams of both fused kernels ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def level_states(oracle):
    """(h, w) -> (R0, R1, flow, M) of one synthetic pair, made once per shape and shared read-only by every window."""
    cache = {}

    def get(h, w):
        if (h, w) not in cache:
            fr = _frames(h * 1000 + w, 2, h, w)
            R0, R1, flow = _level_state(oracle, fr[0], fr[1], 5, 1.1, 6)
            state = (R0, R1, flow, oracle.update_matrices(R0, R1, flow))
            for a in state:
                a.setflags(write=False)
            cache[(h, w)] = state
        return cache[(h, w)]
    return get


def _stage_iterate(ctx, oracle, torch_dev, state, winsize):
    """-> (flow of nsof_stage_iterate on a batch of the same pair twice, the oracle's two stages)."""
    import torch
    R0, R1, flow, M = state
    h, w = flow.shape[:2]
    want, _ = oracle.update_flow_blur(R0, R1, flow, M, winsize, False)
    assert np.isfinite(want).all() and want.any(), (winsize, (h, w))
    Rp = np.stack([np.stack([_rlayout(R0), _rlayout(R1)])] * 2)
    dR, dF = _dev(torch_dev, Rp), _dev(torch_dev, np.stack([flow, flow]))
    out = torch.zeros((2, h, w, 2), dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    ctx.check(ctx._lib.nsof_stage_iterate(ctx.ptr, 2, dR.data_ptr(), dF.data_ptr(), w, h, winsize, out.data_ptr()))
    ctx.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[0], got[1]), (winsize, (h, w), "the two pairs of the batch differ")
    return got[0], want


def _stage_heights(m):
    return (5, 2 * m + 6)   # two 4-row steps, the second partial; a window and a half


@pytest.mark.parametrize("winsize", WINSIZES)
def test_stage_iterate_x_strip_seams(ctx, oracle, torch_dev, level_states, winsize):
    """k_iterate_x<MH, false> over 192-column strips: a last strip of one column (narrower than the halo m), exactly at
    the halo and one past it, and three strips (two hand-overs) -- the oracle's two stages, bit for bit."""
    m = winsize // 2
    for h in _stage_heights(m):
        for w in (193, 192 + m, 192 + m + 1, 385):
            got, want = _stage_iterate(ctx, oracle, torch_dev, level_states(h, w), winsize)
            assert np.array_equal(got, want), (winsize, (h, w), _diff(got, want))


@pytest.mark.parametrize("winsize", WINSIZES)
def test_stage_iterate_q_strip_seams(ctx, oracle, torch_dev, level_states, fast_mode, winsize):
    """k_iterate_q<MH, false> with the frame's right edge one column before, on and one past its strip seam, and on a
    third strip of one column: within float rounding of the oracle's stages (the rule of test_fused_iteration_fast_mode)."""
    m = winsize // 2
    sw = _q_strip(m)
    for h in _stage_heights(m):
        for w in (sw - 1, sw, sw + 1, 2 * sw + 1):
            got, want = _stage_iterate(ctx, oracle, torch_dev, level_states(h, w), winsize)
            d = np.abs(got - want)
            assert d.max() <= 1e-6 * max(1.0, np.abs(want).max()), (winsize, (h, w), float(d.max()))
            assert (got != want).mean() < 0.01, (winsize, (h, w), float((got != want).mean()))


# ---- 2. whole calls: the uniform routes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("winsize", WINSIZES)
def test_uniform_iterate_x(nsof_lib, ctx, oracle, jobs, winsize):
    """k_iterate_x<MH, false>: three pairs of 45 x (192 + m + 1) -- a second strip one column past the halo -- through the
    batch entry, the sequence entry and the lone call, NSOF_OPT_SMALL_BATCH_JOBS = 0."""
    m = winsize // 2
    jobs(0)
    params = _params(winsize)
    shape = (45, 192 + m + 1)
    frames = _frames(300 + winsize, 4, *shape)
    want = [_want_flow(oracle, frames[i], frames[i + 1], params) for i in range(3)]
    (got_b, got_s), counts = _counted(ctx, lambda: _batch_and_sequence(nsof_lib, ctx, frames, params))
    _assert_uniform_route(nsof_lib, counts, "one_kernel", shape, winsize, 2, "batch + sequence")
    for i, wt in enumerate(want):
        assert np.array_equal(got_b[i], wt), (winsize, "batch", i, _diff(got_b[i], wt))
        assert np.array_equal(got_s[i], wt), (winsize, "sequence", i, _diff(got_s[i], wt))
    one, counts = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(frames[0], frames[1], None, *params, ctx=ctx))
    _assert_uniform_route(nsof_lib, counts, "one_kernel", shape, winsize, 1, "lone call")
    assert np.array_equal(one, want[0]), (winsize, "lone call", _diff(one, want[0]))


@pytest.mark.parametrize("winsize", WINSIZES)
def test_uniform_small_batch_four_rows(nsof_lib, ctx, oracle, winsize):
    """k_lat_rowscan<MH, false, 4> and k_lat_colsum<false>: lone calls at the default options.  Heights 63 + m and 64 + m
    lie either side of wave 1's unclamped-load condition (y0 - m - 1 >= 0 && y0 + 32 + m <= H at y0 = 32), 257 is a second
    256-row pass of one row, 33 a second 32-row turn of one row; widths 33 and 32 + m + 1 end just past one 32-column tile
    of the row scan and past its halo, 129 wraps its 128-column ring.  lat_rowscan() takes 4 rows while
    (max_h + 3) / 4 * n <= 256: at most (257 + 3) / 4 * 1 = 65 here."""
    m = winsize // 2
    params = _params(winsize)
    for h in (33, 63 + m, 64 + m, 257):
        for w in (33, 32 + m + 1, 129):
            fr = _frames(h * 1000 + w, 2, h, w)
            want = _want_flow(oracle, fr[0], fr[1], params)
            got, counts = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, *params, ctx=ctx))
            _assert_uniform_route(nsof_lib, counts, "small_batch", (h, w), winsize, 1, "lone call")
            assert np.array_equal(got, want), (winsize, (h, w), _diff(got, want))


@pytest.mark.parametrize("winsize", WINSIZES)
def test_uniform_small_batch_eight_rows(nsof_lib, ctx, oracle, winsize):
    """k_lat_rowscan<MH, false, 8>: five pairs of 205 x 70 at the default options.  5 strip jobs stay under the 64 of
    NSOF_OPT_SMALL_BATCH_JOBS (the small-batch form); at level 0 (205 + 3) / 4 * 5 = 260 > 256, so lat_rowscan() takes 8
    rows, and 205 = 25 * 8 + 5 leaves a partial last workgroup.  Level 1 (102 x 35: 26 * 5 = 130) runs with 4 rows."""
    params = _params(winsize)
    shape = (205, 70)
    frames = _frames(500 + winsize, 6, *shape)
    want = [_want_flow(oracle, frames[i], frames[i + 1], params) for i in range(5)]
    (got_b, got_s), counts = _counted(ctx, lambda: _batch_and_sequence(nsof_lib, ctx, frames, params))
    _assert_uniform_route(nsof_lib, counts, "small_batch", shape, winsize, 2, "batch + sequence")
    for i, wt in enumerate(want):
        assert np.array_equal(got_b[i], wt), (winsize, "batch", i, _diff(got_b[i], wt))
        assert np.array_equal(got_s[i], wt), (winsize, "sequence", i, _diff(got_s[i], wt))
    # the lone call of the first pair: the same form with 4 rows (52 * 1 <= 256)
    one, counts = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(frames[0], frames[1], None, *params, ctx=ctx))
    _assert_uniform_route(nsof_lib, counts, "small_batch", shape, winsize, 1, "lone call")
    assert np.array_equal(one, want[0]), (winsize, "lone call", _diff(one, want[0]))


# ---- 3. work lists ------------------------------------------------------------------------------------------------------------
def _list_shapes(name, m):
    s = [(45, 192 + m + 1), (33, 70), (9, 2 * m + 1), (70, 33), (2, 2), (37, 193)]
    return s if name == "S" else s + [(205, 70), (130, 40)]


def _crops(seed, shapes):
    """Strided views of one frame pair with motion, each at an odd column: [(prev, next), ...]."""
    big = _frames(seed, 2, max(h for h, _ in shapes) + 24, max(w for _, w in shapes) + 40)
    rng = np.random.default_rng(seed)
    out = []
    for (h, w) in shapes:
        y0 = int(rng.integers(0, big.shape[1] - h + 1))
        x0 = int(rng.integers(0, big.shape[2] - w)) | 1
        a, b = big[0, y0:y0 + h, x0:x0 + w], big[1, y0:y0 + h, x0:x0 + w]
        assert a.shape == (h, w) and not a.flags.c_contiguous
        out.append((a, b))
    return out


@pytest.mark.parametrize("name", ["S", "T"])
@pytest.mark.parametrize("winsize", WINSIZES)
def test_work_list_exact_forms(nsof_lib, ctx, oracle, jobs, winsize, name):
    """nsof.farneback_pairs on crops of distinct shapes, each flow the oracle's bits, in both exact forms:
    NSOF_OPT_SMALL_BATCH_JOBS = 0 runs k_iterate_x<MH, true>, 1 << 20 the small-batch form with HET.  lat_rowscan() takes
    4 rows while (max_h + 3) / 4 * n <= 256.  List S (6 items, max_h 70): 18 * 6 = 108, 4 rows at its one level.  List T
    (8 items, max_h 205): 52 * 8 = 416 > 256, 8 rows at level 0; only the 205 x 70 item has a level 1 (102 x 35: 26 * 1,
    4 rows).

    Launch counts.  The work-list driver launches the iteration once per level and iteration for the whole list (the size
    classes split the pyramid and expansion launches only), so with I = 2 iterations the one-kernel form opens
    (Lmax + 1) I K_ITERATE scopes and the small-batch form twice as many: observed 2 and 4 for list S (one level), 4 and 8
    for list T (two levels), at every window; K_BLUR and K_UPDMAT stay 0."""
    from nsof import _lib
    m = winsize // 2
    params = _params(winsize)
    shapes = _list_shapes(name, m)
    pairs = _crops(700 + winsize, shapes)
    want = [_want_flow(oracle, np.ascontiguousarray(a), np.ascontiguousarray(b), params) for a, b in pairs]
    levels = max(nsof_lib.effective_levels(w, h, 0.5, 2) for h, w in shapes) + 1
    assert levels == (1 if name == "S" else 2)
    iterate = {}
    for small_batch in (0, 1 << 20):
        jobs(small_batch)
        flows, counts = _counted(ctx, lambda: nsof_lib.farneback_pairs(pairs, nsof_lib.FarnebackParams(*params), ctx=ctx))
        for i, (f, wt) in enumerate(zip(flows, want)):
            assert np.array_equal(f, wt), (winsize, name, small_batch, shapes[i], _diff(f, wt))
        assert counts[_lib.K_BLUR] == 0 and counts[_lib.K_UPDMAT] == 0, (winsize, name, small_batch, counts)
        iterate[small_batch] = counts[_lib.K_ITERATE]
    assert iterate[0] == levels * ITERATIONS, (winsize, name, iterate)
    assert iterate[1 << 20] == 2 * iterate[0], (winsize, name, iterate)


@pytest.mark.parametrize("winsize", WINSIZES)
def test_work_list_fast_mode(nsof_lib, ctx, oracle, fast_mode, winsize):
    """k_iterate_q<MH, true>: a list with an item one column past the strip seam and one of three strips whose last has
    one column, and k_iterate_q<MH, false> on the lone call of the first item: within the pipeline rule of the fuzz
    sweep.  One K_ITERATE scope per level and iteration (observed 2 for the list and for the lone call), no K_BLUR."""
    from nsof import _lib
    m = winsize // 2
    sw = _q_strip(m)
    params = _params(winsize)
    shapes = [(37, sw + 1), (21, 2 * sw + 1), (33, 70), (9, 2 * m + 1)]
    pairs = _crops(900 + winsize, shapes)
    want = [_want_flow(oracle, np.ascontiguousarray(a), np.ascontiguousarray(b), params) for a, b in pairs]
    assert max(nsof_lib.effective_levels(w, h, 0.5, 2) for h, w in shapes) == 0

    def check(got, wt, tag):
        err = float(np.abs(got - wt).max())
        assert err <= PIPE_TOL * max(1.0, float(np.abs(wt).max()) / 10), (winsize, tag, err)

    flows, counts = _counted(ctx, lambda: nsof_lib.farneback_pairs(pairs, nsof_lib.FarnebackParams(*params), ctx=ctx))
    assert counts[_lib.K_ITERATE] == ITERATIONS and counts[_lib.K_BLUR] == 0 and counts[_lib.K_UPDMAT] == 0, (winsize, counts)
    for i, (f, wt) in enumerate(zip(flows, want)):
        check(f, wt, shapes[i])
    a, b = (np.ascontiguousarray(x) for x in pairs[0])
    one, counts = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(a, b, None, *params, ctx=ctx))
    assert counts[_lib.K_ITERATE] == ITERATIONS and counts[_lib.K_BLUR] == 0 and counts[_lib.K_UPDMAT] == 0, (winsize, counts)
    check(one, want[0], "lone call")
