"""GPU: cycle-to-cycle write noise and the pair-index origin of the frame-driven array run (``nsof_accum_frames_f64_c2c*``,
``simulate_frames*(trials=, c2c=, first_pair=)``, ``pipeline.gating_variability_dev(c2c=)``).  Without noise every entry gives
the bits it gave before; with noise the run is pinned to the NumPy restatement ``frames_c2c_ref`` -- bit for bit on a device
that takes no power, within twice the project's noiseless bounds on the three class devices -- and to itself: a trial does not
depend on how many trials run, nor a pair on how the video is cut into calls.  tests/test_frames_c2c_cpu.py asserts the
conditions on these inputs without which a test here could pass vacuously."""
import ctypes as C

import numpy as np
import pytest

import accum_params_ref as R
import frames_c2c_ref as Z  # noqa: N812
from test_frames_dev_gpu import GUARD, SENTINEL, _array_case, _guarded
from test_frames_maps_gpu import _class_planes, _labels

pytestmark = pytest.mark.gpu

DT, N_SUB = Z.DT, Z.N_SUB
TH = Z.THRESHOLDS[0]
QUIET_FORMS = [dict(first_pair=7), dict(c2c=dict(sigma=0.0, seed=9)), dict(c2c=dict(sigma_on=0, sigma_off=0))]


def _dev(imgs, torch_dev):
    import torch
    d = torch.from_numpy(np.ascontiguousarray(imgs)).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    return d


def _run(nsof_lib, ctx, d, th=TH, n_sub=N_SUB, **kw):
    """``simulate_frames_dev`` -> (w, res, cur) as NumPy arrays."""
    out = nsof_lib.simulate_frames_dev(d, DT, n_sub, th[0], th[1], ctx=ctx, **kw)
    ctx.synchronize()
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("grid", Z.GRIDS)
def test_the_frames_are_those_of_the_array_case(nsof_lib, ctx, grid):
    assert np.array_equal(Z.frames(grid), _array_case(nsof_lib, ctx, grid, TH)[0])


@pytest.mark.parametrize("trials", [1, 3])
@pytest.mark.parametrize("th", Z.THRESHOLDS)
@pytest.mark.parametrize("grid", Z.GRIDS)
def test_noise_off_is_the_run_without_the_new_keywords(nsof_lib, ctx, torch_dev, grid, th, trials):
    d = _dev(Z.frames(grid), torch_dev)
    planes = _class_planes(_labels(grid[0] * 7 + trials, (trials,) + grid))
    for params in (None, Z.CLASSES[0]):                  # the fitted device; a device in the kernel arguments
        base = _run(nsof_lib, ctx, d, th, params=params)
        mapped = _run(nsof_lib, ctx, d, th, params=params, param_maps=planes)
        assert mapped[0].shape == (trials,) + grid
        for quiet in QUIET_FORMS:
            got = _run(nsof_lib, ctx, d, th, params=params, param_maps=planes, **quiet)          # planes
            assert all(np.array_equal(g, m) for g, m in zip(got, mapped)), quiet
            got = _run(nsof_lib, ctx, d, th, params=params, param_maps=planes, trials=trials, **quiet)
            assert all(np.array_equal(g, m) for g, m in zip(got, mapped)), quiet
            got = _run(nsof_lib, ctx, d, th, params=params, **quiet)                             # no planes, no trial axis
            assert all(g.shape == b.shape and np.array_equal(g, b) for g, b in zip(got, base)), quiet
            got = _run(nsof_lib, ctx, d, th, params=params, trials=trials, **quiet)              # no planes, T trials alike
            assert got[0].shape == (trials,) + grid
            assert all(np.array_equal(g[t], b) for g, b in zip(got, base) for t in range(trials)), quiet


@pytest.mark.parametrize("grid", Z.GRIDS)
def test_noise_plumbing_bit_for_bit(nsof_lib, ctx, torch_dev, grid):
    """A device without a power: counter layout, branch choice, clamp and operation order, independent of the device pow."""
    imgs, planes, want = Z.pow_free_case(grid)
    w, res, cur = _run(nsof_lib, ctx, _dev(imgs, torch_dev), params=Z.POW_FREE, param_maps=planes, c2c=Z.NOISE)
    assert w.shape == (3,) + grid and res.shape == (3, 5) + grid and cur.shape == (3, 4) + grid
    assert np.array_equal(w, want["w"][-1])
    assert np.array_equal(cur, 1.0 / res[:, 1:])
    want_res = np.moveaxis(want["res"], 0, 1)            # [T][n][H][W]
    err = (np.abs(res - want_res) / want_res).max()
    print(f"{grid}: max rel res error {err:.3g} (bound 1e-12)")
    assert err <= 1e-12
    quiet = _run(nsof_lib, ctx, _dev(imgs, torch_dev), params=Z.POW_FREE, param_maps=planes)
    assert not np.array_equal(quiet[0], w)


@pytest.mark.parametrize("grid,n_sub", Z.CLASS_CASES)
def test_real_devices_against_the_restatement(nsof_lib, ctx, torch_dev, grid, n_sub):
    """Twice the noiseless bounds of test_frames_maps_gpu.test_against_the_restatement (1e-12 at n_sub 10, 1e-9 at n_sub 1000):
    with sigma <= 0.1 the step is scaled by at most 1 + 6.90 * 0.1 < 2."""
    tol = 2 * (1e-12 if n_sub == 10 else 1e-9)
    imgs, planes, noisy, quiet = Z.class_case(grid, n_sub)
    d = _dev(imgs, torch_dev)
    errs = []
    for want, kw in ((noisy, dict(c2c=Z.NOISE)), (quiet, {})):
        w, res, _ = _run(nsof_lib, ctx, d, n_sub=n_sub, param_maps=planes, **kw)
        want_res = np.moveaxis(want["res"], 0, 1)
        errs.append((np.abs(w - want["w"][-1]).max(), (np.abs(res - want_res) / want_res).max()))
    (ew, er), (qw, qr) = errs
    print(f"{grid} n_sub {n_sub}: max |w - restatement| {ew:.3g}, max rel res {er:.3g} (bound {tol:g}); without noise {qw:.3g}, {qr:.3g}")
    assert ew <= tol and er <= tol


def test_clamp(nsof_lib, ctx, torch_dev):
    """One pair, sigma = 1000: a pulse whose factor would be negative does not switch at all."""
    imgs, _ = Z.clamp_case()
    seed, grid, T = Z.CLAMP_NOISE["seed"], (13, 24), 5  # noqa: N806
    xi = np.array([[nsof_lib.c2c_noise(seed, 0, t, i, 0, 1)[0] for i in range(312)] for t in range(T)]).reshape((T,) + grid)
    u = 1.0 + np.float64(np.float32(1000.0)) * xi.astype(np.float64)
    assert (u < 0).sum() > 100 and (u > 0).sum() > 100
    w, res, _ = _run(nsof_lib, ctx, _dev(imgs, torch_dev), trials=T, c2c=Z.CLAMP_NOISE)
    assert w.shape == (T,) + grid
    assert (w[u < 0] == R.DEFAULT["wini"]).all() and (w[u > 0] != R.DEFAULT["wini"]).all()


@pytest.mark.parametrize("which", ["on", "off"])
def test_direction(nsof_lib, ctx, torch_dev, which):
    """Noise on one branch only: cells whose pair took the other branch or the dead zone keep the noiseless bits."""
    imgs, planes, want, _ = Z.direction_case(which)
    d = _dev(imgs, torch_dev)
    noise = Z.ON_ONLY if which == "on" else Z.OFF_ONLY
    quiet = _run(nsof_lib, ctx, d, params=Z.QUIET, param_maps=planes, trials=2)
    noisy = _run(nsof_lib, ctx, d, params=Z.QUIET, param_maps=planes, trials=2, c2c=noise)
    sel = want["on" if which == "on" else "off"][0] & (want["xi"][0] != 0)
    assert sel.sum() > 50 and (~sel).sum() > 50
    for a, b in ((noisy[0], quiet[0]), (noisy[1][:, 1], quiet[1][:, 1]), (noisy[2][:, 0], quiet[2][:, 0])):   # w, res, cur
        assert np.array_equal(a[~sel], b[~sel]) and (a[sel] != b[sel]).all()


@pytest.mark.parametrize("grid", [(4, 4), (13, 24)])
def test_independence(nsof_lib, ctx, torch_dev, grid):
    imgs = Z.frames(grid)
    d = _dev(imgs, torch_dev)
    # a trial does not depend on how many trials run: without planes ...
    five = _run(nsof_lib, ctx, d, trials=5, c2c=Z.NOISE)
    three = _run(nsof_lib, ctx, d, trials=3, c2c=Z.NOISE)
    assert five[0].shape == (5,) + grid and not np.array_equal(five[0][0], five[0][1])
    assert all(np.array_equal(a[:3], b) for a, b in zip(five, three))
    # ... and with [T][H][W] planes
    planes5 = _class_planes(_labels(11, (5,) + grid))
    planes3 = {k: v[:3] for k, v in planes5.items()}
    five_p = _run(nsof_lib, ctx, d, param_maps=planes5, c2c=Z.NOISE)
    three_p = _run(nsof_lib, ctx, d, param_maps=planes3, c2c=Z.NOISE)
    assert all(np.array_equal(a[:3], b) for a, b in zip(five_p, three_p)) and not np.array_equal(five_p[0], five[0])
    # c2c alone runs trial 0 and returns the shapes of the call without it
    alone = _run(nsof_lib, ctx, d, c2c=Z.NOISE)
    assert alone[0].shape == grid and all(np.array_equal(a, b[0]) for a, b in zip(alone, five))
    # a video cut into two calls: frames [0:3], then frames [2:5] from the first call's state with first_pair = 2
    for kw, one in ((dict(trials=5), five), (dict(param_maps=planes3), three_p)):
        head = _run(nsof_lib, ctx, _dev(imgs[:3], torch_dev), c2c=Z.NOISE, **kw)
        maps = dict(kw.get("param_maps", {}), wini=head[0])
        tail = _run(nsof_lib, ctx, _dev(imgs[2:], torch_dev), c2c=Z.NOISE, first_pair=2, param_maps=maps)
        assert np.array_equal(head[1], one[1][:, :3]) and np.array_equal(head[2], one[2][:, :2])
        assert np.array_equal(tail[0], one[0]) and np.array_equal(tail[1][:, 1:], one[1][:, 3:])
        assert np.array_equal(tail[2], one[2][:, 2:])
        again = _run(nsof_lib, ctx, _dev(imgs[2:], torch_dev), c2c=Z.NOISE, first_pair=0, param_maps=maps)
        assert not np.array_equal(again[0], one[0])      # the origin matters
    # the host entry equals the device entry
    hw, hres = nsof_lib.simulate_frames(imgs, DT, N_SUB, TH[0], TH[1], ctx=ctx, param_maps=planes3, c2c=Z.NOISE)
    assert np.array_equal(hw, three_p[0]) and np.array_equal(hres, three_p[1])
    hw, hres = nsof_lib.simulate_frames(imgs[2:], DT, N_SUB, TH[0], TH[1], ctx=ctx, c2c=Z.NOISE, first_pair=2)
    d_tail = _run(nsof_lib, ctx, _dev(imgs[2:], torch_dev), c2c=Z.NOISE, first_pair=2)
    assert hw.shape == grid and np.array_equal(hw, d_tail[0]) and np.array_equal(hres, d_tail[1])
    # two seeds give two results
    other = _run(nsof_lib, ctx, d, trials=3, c2c=dict(Z.NOISE, seed=Z.NOISE["seed"] + 1))
    assert not np.array_equal(other[0], three[0])


def test_refusals_leave_the_outputs_untouched(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import _lib
    from nsof.accumulator import accum_params
    ap = accum_params(None)
    keys, planes, counts = (C.c_int * 1)(), (C.c_void_p * 1)(), (C.c_int * 1)()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def status(grid, trials, c2c, first_pair, n=3):
        """The raw device entry on guarded buffers large enough for the call it refuses -> (status, message, sentinels intact)."""
        d = _dev(np.full((n,) + grid, 0.5), torch_dev)
        bufs = [_guarded(torch, torch_dev, s) for s in ((trials,) + grid, (trials, n) + grid, (trials, n - 1) + grid)]
        torch.cuda.synchronize(torch_dev)
        nz = None if c2c is None else C.byref(_lib.AccumC2c(*c2c))
        rc = ctx._lib.nsof_accum_frames_f64_c2c_dev(ctx.ptr, ptr(d), n, grid[0], grid[1], DT, N_SUB, TH[0], TH[1], 1.0, C.byref(ap),
                                                    trials, 0, keys, planes, counts, *[ptr(t) for _, t in bufs], nz, first_pair)
        msg = (ctx._lib.nsof_last_error(ctx.ptr) or b"").decode()
        ctx.synchronize()
        assert all(bool((b[-GUARD:] == SENTINEL).all()) for b, _ in bufs)              # nothing is ever written behind an output
        return rc, msg, all(bool((b == SENTINEL).all()) for b, _ in bufs)

    rc, msg, intact = status((4, 4), 2, (5, 0.05, 0.1), 0)                     # the accepted call writes: the guards alone stay
    assert rc == 0 and not intact, msg
    for c2c, first_pair, grid, trials, want, named in (
            ((5, -0.1, 0.1), 0, (4, 4), 2, _lib.NSOF_EINVAL, "sigma_on"),
            ((5, 0.1, float("nan")), 0, (4, 4), 2, _lib.NSOF_EINVAL, "sigma_off"),
            ((5, float("inf"), 0.0), 0, (4, 4), 2, _lib.NSOF_EINVAL, "sigma_on"),
            ((5, 0.05, 0.1), -1, (4, 4), 2, _lib.NSOF_EINVAL, "first_pair"),
            (None, -1, (4, 4), 2, _lib.NSOF_EINVAL, "first_pair"),
            ((5, 0.05, 0.1), 2**63 - 2, (4, 4), 2, _lib.NSOF_EINVAL, "first_pair"),   # first_pair + n_frames overflows
            ((5, 0.05, 0.1), 0, (1, 1), 65536, _lib.NSOF_EUNSUPPORTED, "n_trials")):
        rc, msg, intact = status(grid, trials, c2c, first_pair)
        assert rc == want and named in msg and intact, (c2c, first_pair, trials, rc, msg)
    assert "-0.1" in status((4, 4), 2, (5, -0.1, 0.1), 0)[1]                   # the value is named too
    # 65536 trials without noise are no refusal: the trial word is not drawn from
    rc, msg, intact = status((1, 1), 65536, (5, 0.0, 0.0), 0)
    assert rc == 0 and not intact, msg
    # the host twin refuses the same way, its outputs untouched
    imgs = np.full((3, 4, 4), 0.5)
    hw, hres = np.full((2, 4, 4), SENTINEL), np.full((2, 3, 4, 4), SENTINEL)
    for c2c, first_pair, named in (((5, -0.1, 0.1), 0, "sigma_on"), ((5, 0.1, 0.1), -1, "first_pair")):
        rc = ctx._lib.nsof_accum_frames_f64_c2c(ctx.ptr, imgs.ctypes.data, 3, 4, 4, DT, N_SUB, TH[0], TH[1], C.byref(ap), 2, 0, keys,
                                                planes, counts, hw.ctypes.data, hres.ctypes.data, C.byref(_lib.AccumC2c(*c2c)),
                                                first_pair)
        assert rc == _lib.NSOF_EINVAL and named.encode() in ctx._lib.nsof_last_error(ctx.ptr)
        assert (hw == SENTINEL).all() and (hres == SENTINEL).all()


def _clip_frames():
    """Six 64 x 96 BGR frames: a bright 20 x 28 patch moves 9 px right and 4 px down per frame over static texture."""
    rng = np.random.default_rng(17)
    texture = rng.integers(40, 120, (64, 96, 3), dtype=np.uint8)
    out = []
    for f in range(6):
        fr = texture.copy()
        fr[5 + 4 * f:5 + 4 * f + 20, 6 + 9 * f:6 + 9 * f + 28] = 250
        out.append(fr)
    return np.stack(out)


def test_join_variability_with_noise(nsof_lib, ctx, torch_dev):
    """6 frames of 64 x 96, MEMSIZE 16 (a 4 x 6 grid), n_sub_steps 20, 3 trials."""
    import torch
    from nsof import gating, pipeline
    from nsof.accumulator import variability_maps
    from test_gate_stats_gpu import SPREAD, THRES
    cfg = gating.GatingConfig(MEMSIZE=16, THRES=THRES, OFFSET=0)
    d_bgr = torch.from_numpy(_clip_frames()).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    T, noise = 3, dict(sigma_on=0.05, sigma_off=0.1, seed=41)  # noqa: N806
    nominal = pipeline.gating_stack_from_frames_dev(d_bgr, cfg, n_sub_steps=20, ctx=ctx)
    assert nominal.shape == (5, 4, 6)
    # identical devices that differ by their noise alone: the trial run is taken also with an empty rel_sigma
    out = pipeline.gating_variability_dev(d_bgr, cfg, {}, T, n_sub_steps=20, ctx=ctx, c2c=noise)
    assert torch.equal(out["nominal"], nominal)          # the nominal array stays noiseless
    direct = pipeline.gating_stack_from_frames_dev(d_bgr, cfg, n_sub_steps=20, ctx=ctx, trials=T, c2c=noise)
    assert out["stacks"].shape == (T, 5, 4, 6) and torch.equal(out["stacks"], direct)
    for a in range(T):
        assert not torch.equal(out["stacks"][a], nominal)
        for b in range(a):
            assert not torch.equal(out["stacks"][a], out["stacks"][b])
    stacks = out["stacks"].cpu().numpy()
    counts, flips = gating.gate_stats(stacks, nominal.cpu().numpy(), THRES)
    assert np.array_equal(out["counts"].cpu().numpy(), counts) and np.array_equal(out["flips"].cpu().numpy(), flips)
    assert out["p_gate"].dtype == torch.float64 and np.array_equal(out["p_gate"].cpu().numpy(), counts / T)
    # without c2c an empty rel_sigma still repeats the nominal stack
    plain = pipeline.gating_variability_dev(d_bgr, cfg, {}, T, n_sub_steps=20, ctx=ctx)
    assert all(torch.equal(plain["stacks"][t], nominal) for t in range(T))
    # spreads and noise together: the direct call with the planes of the study
    both = pipeline.gating_variability_dev(d_bgr, cfg, SPREAD, T, seed=3, n_sub_steps=20, ctx=ctx, c2c=noise)
    grids = pipeline._compressed_grids_dev(d_bgr, cfg, None, None, None, ctx, "test")
    maps = variability_maps(4, 6, SPREAD, None, 3, trials=T, dtype=np.float64)
    want = nsof_lib.simulate_frames_dev(grids, n_sub_steps=20, ctx=ctx, param_maps=maps, c2c=noise)[2]
    ctx.synchronize()
    assert torch.equal(both["stacks"], want) and not torch.equal(both["stacks"], out["stacks"])
    assert torch.equal(both["nominal"], nominal)
