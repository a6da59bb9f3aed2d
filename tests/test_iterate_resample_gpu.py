"""The exact iteration that resamples the coarser level's flow as it fetches it (k_iterate_xr, FlowResample2x).

On an exact doubling the first iteration of a pyramid level reads the COARSER level's flow and forms resize(INTER_LINEAR)
x (1 / pyr_scale) per fetched pixel, so the level needs no flow-resample launch.  It must compute what the two kernels
compute -- nsof_stage_flow_upsample, then nsof_stage_iterate -- bit for bit: at every window size (each MH is its own
instance, and its parity picks the row pairing of the resampling walk), over one, two and three strips, over steps with
clamped rows, with samples inside and outside the image, on non-finite input, and with a factor 1 / pyr_scale that is not
a power of two (0.501, 0.499: the levels of 0.5, an inexact product).  The driver takes it only where it is
that computation: the scope counters show which launches a call made.
"""
import numpy as np
import pytest

from test_exact_paths_gpu import _diff, _frames, jobs  # noqa: F401  (jobs is a fixture)
from test_farneback_gpu import _dev, _rlayout

pytestmark = pytest.mark.gpu

WINSIZES = list(range(2, 16))
A = (0.5, 3, 15, 3, 5, 1.2, 0)
# 1 / 0.5 is a power of two, so the resampled field's final product with it is exact and its place in the blend does not
# show; 0.501 and 0.499 give a 272 x 400 frame the level sizes of 0.5 and a factor with a non-zero mantissa
# (tests/test_float_reference.py checks both without a GPU)
PYR_SCALES = (0.5, 0.501, 0.499)


def _shapes(m):
    """(h, w): heights of two steps (the second partial) and of a window and a half; widths of one strip, of a last strip
    of two columns (narrower than the halo), of a last strip one column past the halo, and of two hand-overs."""
    past_halo = 192 + m + 1
    past_halo += past_halo & 1
    return [(h, w) for h in (6, 2 * m + 6) for w in (64, 194, past_halo, 386)]


def _coarse_flow(seed, ph, pw):
    """Two coarse fields (ph, pw, 2): a ramp through zero plus noise.  Doubled, it pushes the samples of the outer columns
    and of the first and last rows out of the image and leaves the middle inside."""
    rng = np.random.default_rng(seed)
    ys, xs = np.meshgrid(np.linspace(-1, 1, ph), np.linspace(-1, 1, pw), indexing="ij")
    out = []
    for amp in (2.0, 1.3):   # one field per pair of the batch
        u = amp * xs + 0.15 * rng.standard_normal((ph, pw))
        v = 0.8 * ys + 0.15 * rng.standard_normal((ph, pw))
        out.append(np.stack([u, v], -1).astype(np.float32))
    return np.stack(out)


def _inside(flow):
    """FarnebackUpdateMatrices' test of a sample, on the CPU -> ((h, w) bool, samples exist beyond [left, right, top,
    bottom])."""
    h, w = flow.shape[:2]
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float32), np.arange(w, dtype=np.float32), indexing="ij")
    x1, y1 = np.floor(xs + flow[..., 0]), np.floor(ys + flow[..., 1])
    sides = [bool((x1 < 0).any()), bool((x1 > w - 2).any()), bool((y1 < 0).any()), bool((y1 > h - 2).any())]
    return (x1 >= 0) & (x1 <= w - 2) & (y1 >= 0) & (y1 <= h - 2), sides


@pytest.fixture(scope="module")
def level_inputs(oracle):
    """(h, w) -> (R0, R1, coarse flows [2]) of one synthetic pair, made once per shape, read-only."""
    cache = {}

    def get(h, w):
        if (h, w) not in cache:
            fr = _frames(h * 1000 + w, 2, h, w)
            R0 = oracle.polyexp(oracle.pyr_level(fr[0], 0.5, 0), 5, 1.1)
            R1 = oracle.polyexp(oracle.pyr_level(fr[1], 0.5, 0), 5, 1.1)
            state = (R0, R1, _coarse_flow(h * 7 + w, h // 2, w // 2))
            for a in state:
                a.setflags(write=False)
            cache[(h, w)] = state
        return cache[(h, w)]
    return get


def _both_paths(ctx, torch_dev, R0, R1, coarse, h, w, winsize, pyr_scale):
    """-> (the resampling iteration, flow_upsample then iterate) of a batch of two pairs with the same R; both multiply the
    resampled field by float(1 / pyr_scale)."""
    import torch
    lib = ctx._lib
    Rp = np.stack([np.stack([_rlayout(R0), _rlayout(R1)])] * 2)
    dR, dC = _dev(torch_dev, Rp), _dev(torch_dev, coarse)
    up = torch.zeros((2, h, w, 2), dtype=torch.float32, device=torch_dev)
    two = torch.zeros_like(up)
    one = torch.zeros_like(up)
    torch.cuda.synchronize()
    ctx.check(lib.nsof_stage_flow_upsample(ctx.ptr, 2, dC.data_ptr(), w // 2, h // 2, up.data_ptr(), w, h, pyr_scale))
    ctx.check(lib.nsof_stage_iterate(ctx.ptr, 2, dR.data_ptr(), up.data_ptr(), w, h, winsize, two.data_ptr()))
    ctx.check(lib.nsof_stage_iterate_x_resample(ctx.ptr, 2, dR.data_ptr(), dC.data_ptr(), w // 2, h // 2, w, h, winsize,
                                                pyr_scale, one.data_ptr()))
    ctx.synchronize()
    return one.cpu().numpy(), two.cpu().numpy()


@pytest.mark.parametrize("pyr_scale,winsize", [(ps, ws) for ps in PYR_SCALES for ws in WINSIZES],
                         ids=[(f"{ws}" if ps == 0.5 else f"{ws}-ps{ps}") for ps in PYR_SCALES for ws in WINSIZES])
def test_stage_resample_equals_two_kernels_and_oracle(ctx, oracle, torch_dev, level_inputs, pyr_scale, winsize):
    """At pyr_scale 0.5 the factor is 2 and the product with it exact, whatever its place in the blend; at 0.501 and 0.499
    it is not, and (t0*b0 + t1*b1) * mul, t0*(b0*mul) + t1*(b1*mul) and a contracted product give different bits."""
    m = winsize // 2
    for (h, w) in _shapes(m):
        R0, R1, coarse = level_inputs(h, w)
        one, two = _both_paths(ctx, torch_dev, R0, R1, coarse, h, w, winsize, pyr_scale)
        for i in range(2):
            fine = oracle.resize_linear(coarse[i], w, h) * np.float32(1.0 / pyr_scale)
            ins, sides = _inside(fine)
            assert ins.any() and not ins.all(), (winsize, (h, w), i, "both values of `inside` must occur")
            assert all(sides), (winsize, (h, w), i, "samples must leave the image on every side", sides)
            want, _ = oracle.update_flow_blur(R0, R1, fine, oracle.update_matrices(R0, R1, fine), winsize, False)
            assert np.isfinite(want).all() and want.any(), (winsize, (h, w), i)
            assert np.array_equal(one[i], two[i]), (winsize, (h, w), i, "two kernels", _diff(one[i], two[i]))
            assert np.array_equal(one[i], want), (winsize, (h, w), i, "oracle", _diff(one[i], want))


@pytest.mark.parametrize("pyr_scale", PYR_SCALES)
def test_stage_resample_non_finite_input(ctx, oracle, torch_dev, level_inputs, pyr_scale):
    """A NaN and a +inf in the coarse field, the inf in the last coarse column (whose right neighbour is the clamped
    column itself, weight 0: 0 x inf must still be formed).  The bits of the two-kernel path, at every factor."""
    h, w, winsize = 20, 194, 15
    R0, R1, coarse = level_inputs(h, w)
    coarse = coarse.copy()
    coarse[0, 3, 40, 0] = np.nan
    coarse[0, 6, w // 2 - 1, 1] = np.inf
    coarse[1, 9, w // 2 - 1, 0] = np.nan
    coarse[1, 0, 0, 1] = np.inf
    one, two = _both_paths(ctx, torch_dev, R0, R1, coarse, h, w, winsize, pyr_scale)
    assert not np.isfinite(two).all(), "the non-finite input must reach the result"
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32)), _diff(one, two)


@pytest.mark.parametrize("fine,src,winsize", [((21, 195), (10, 97), 15), ((20, 194), (10, 97), 17)],
                         ids=["not_a_doubling", "winsize17"])
def test_stage_resample_refuses(ctx, torch_dev, fine, src, winsize):
    import torch
    from nsof import _lib
    (h, w), (sh, sw) = fine, src
    R = torch.zeros((1, 2, 5 * h * w), dtype=torch.float32, device=torch_dev)
    coarse = torch.ones((1, sh, sw, 2), dtype=torch.float32, device=torch_dev)
    out = torch.full((1, h, w, 2), 7.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    rc = ctx._lib.nsof_stage_iterate_x_resample(ctx.ptr, 1, R.data_ptr(), coarse.data_ptr(), sw, sh, w, h, winsize, 0.5,
                                                out.data_ptr())
    assert rc == _lib.NSOF_EUNSUPPORTED
    ctx.synchronize()
    assert bool((out == 7.0).all())


# ---- whole calls ---------------------------------------------------------------------------------------------------------
def _counted(ctx, call):
    """Runs `call` -> (its result, K_UPSAMPLE scopes, K_ITERATE scopes)."""
    from nsof import _lib
    ids = (_lib.K_UPSAMPLE, _lib.K_ITERATE)
    ctx.prof_enable(*ids)
    try:
        for k in ids:
            ctx.prof_collect(k)
        out = call()
        ctx.synchronize()
        return (out,) + tuple(ctx.prof_collect(k)[1] for k in ids)
    finally:
        ctx.prof_enable()


def _transitions(nsof_lib, h, w, params):
    """-> (levels below the coarsest, how many of them are not an exact doubling of the level above them)."""
    L = nsof_lib.effective_levels(w, h, params[0], params[1])
    size = [nsof_lib.level_size(w, h, params[0], k)[:2] for k in range(L + 1)]
    inexact = sum(1 for k in range(L) if (size[k][0], size[k][1]) != (2 * size[k + 1][0], 2 * size[k + 1][1]))
    return L, inexact


def test_whole_call_exact_doublings(nsof_lib, ctx, oracle, jobs):
    """2 pairs of 272 x 400, parameter set A: levels 400 / 200 / 100 / 50 wide (three strips, two, one, one), every one the
    double of the next: no resample launch, 4 x 3 iterations, the oracle's bits -- batch entry and sequence entry."""
    import torch
    jobs(0)
    h, w = 272, 400
    assert _transitions(nsof_lib, h, w, A) == (3, 0)
    frames = _frames(4242, 3, h, w)
    want = [oracle.farneback(frames[i], frames[i + 1], *A) for i in range(2)]
    assert all(np.isfinite(x).all() and np.abs(x).max() > 1.0 for x in want)
    P = nsof_lib.FarnebackParams(*A)
    dev = torch.device("cuda", 0)
    dp, dn = torch.from_numpy(frames[:-1].copy()).to(dev), torch.from_numpy(frames[1:].copy()).to(dev)
    ds = torch.from_numpy(frames).to(dev)
    fb = torch.empty((2, h, w, 2), dtype=torch.float32, device=dev)
    fs = torch.empty_like(fb)
    torch.cuda.synchronize()
    _, ups, its = _counted(ctx, lambda: nsof_lib.farneback_batch(dp, dn, fb, 2, h, w, P, ctx=ctx))
    assert (ups, its) == (0, 12), ("batch", ups, its)
    _, ups, its = _counted(ctx, lambda: nsof_lib.farneback_sequence(ds, fs, 3, h, w, P, ctx=ctx))
    assert (ups, its) == (0, 12), ("sequence", ups, its)
    got_b, got_s = fb.cpu().numpy(), fs.cpu().numpy()
    for i in range(2):
        assert np.array_equal(got_b[i], want[i]), ("batch", i, _diff(got_b[i], want[i]))
        assert np.array_equal(got_s[i], want[i]), ("sequence", i, _diff(got_s[i], want[i]))


@pytest.mark.parametrize("pyr_scale,winsize", [(0.501, 15), (0.499, 15), (0.501, 4)])
def test_whole_call_exact_doublings_at_other_scales(nsof_lib, ctx, oracle, jobs, pyr_scale, winsize):
    """The same 2 pairs of 272 x 400 at pyr_scale 0.501 and 0.499: the levels are still 400 / 200 / 100 / 50 by 272 / 136 /
    68 / 34, so every level takes the resampling first iteration -- with the factor float(1 / pyr_scale), which is not a
    power of two.  No resample launch, 4 x 3 iterations, the oracle's bits, batch entry and sequence entry; window 4 runs
    an even-MH instance (MH = 2) inside a whole call beside window 15's odd one."""
    import torch
    jobs(0)
    h, w = 272, 400
    params = (pyr_scale, 3, winsize, 3, 5, 1.2, 0)
    assert _transitions(nsof_lib, h, w, params) == (3, 0)
    frames = _frames(4242, 3, h, w)
    want = [oracle.farneback(frames[i], frames[i + 1], *params) for i in range(2)]
    assert all(np.isfinite(x).all() and np.abs(x).max() > 1.0 for x in want)
    P = nsof_lib.FarnebackParams(*params)
    dev = torch.device("cuda", 0)
    dp, dn = torch.from_numpy(frames[:-1].copy()).to(dev), torch.from_numpy(frames[1:].copy()).to(dev)
    ds = torch.from_numpy(frames).to(dev)
    fb = torch.empty((2, h, w, 2), dtype=torch.float32, device=dev)
    fs = torch.empty_like(fb)
    torch.cuda.synchronize()
    _, ups, its = _counted(ctx, lambda: nsof_lib.farneback_batch(dp, dn, fb, 2, h, w, P, ctx=ctx))
    assert (ups, its) == (0, 12), ("batch", ups, its)
    _, ups, its = _counted(ctx, lambda: nsof_lib.farneback_sequence(ds, fs, 3, h, w, P, ctx=ctx))
    assert (ups, its) == (0, 12), ("sequence", ups, its)
    got_b, got_s = fb.cpu().numpy(), fs.cpu().numpy()
    for i in range(2):
        assert np.array_equal(got_b[i], want[i]), ("batch", i, _diff(got_b[i], want[i]))
        assert np.array_equal(got_s[i], want[i]), ("sequence", i, _diff(got_s[i], want[i]))


def test_whole_call_inexact_level_keeps_its_resample(nsof_lib, ctx, oracle, jobs):
    """200 x 303: level 1 is 152 wide, so level 0 is not its double and keeps the resample launch."""
    jobs(0)
    h, w = 200, 303
    L, inexact = _transitions(nsof_lib, h, w, A)
    assert L >= 2 and 1 <= inexact < L
    fr = _frames(777, 2, h, w)
    want = oracle.farneback(fr[0], fr[1], *A)
    got, ups, its = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, *A, ctx=ctx))
    assert (ups, its) == (inexact, (L + 1) * A[3]), (ups, its, L, inexact)
    assert np.array_equal(got, want), _diff(got, want)


def test_whole_call_fma_variant_keeps_two_kernels(nsof_lib, ctx, jobs):
    """NSOF_OPT_PYR_FMA blends with one rounding, which the resampling source does not do: every level keeps its resample
    launch, and the one-kernel form gives the bits of the small-batch form (which never resamples in the iteration)."""
    from nsof import _lib
    h, w = 272, 400
    fr = _frames(4242, 2, h, w)
    saved = ctx.get_option(_lib.OPT_PYR_FMA)
    ctx.set_option(_lib.OPT_PYR_FMA, 1)
    try:
        ref, ups_ref, _ = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, *A, ctx=ctx))
        jobs(0)
        got, ups, its = _counted(ctx, lambda: nsof_lib.calcOpticalFlowFarneback(fr[0], fr[1], None, *A, ctx=ctx))
    finally:
        ctx.set_option(_lib.OPT_PYR_FMA, saved)
    assert (ups_ref, ups, its) == (3, 3, 12), (ups_ref, ups, its)
    assert np.array_equal(got, ref), _diff(got, ref)
