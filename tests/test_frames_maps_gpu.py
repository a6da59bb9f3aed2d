"""GPU: the frame-driven array run with a device model per cell and per trial (``nsof_accum_frames_f64_maps*``,
``simulate_frames*(param_maps=)``).  Every (trial, cell) is pinned bit for bit to the uniform entries at that cell's
parameters -- the code that ran before maps existed -- and, within the bounds of
``test_accum_params_gpu.test_frame_driven_run_with_parameters``, to the NumPy restatement ``accum_params_ref``."""
import ctypes as C

import numpy as np
import pytest

import accum_params_ref as R
from test_frames_dev_gpu import GUARD, SENTINEL, _array_case, _guarded

pytestmark = pytest.mark.gpu

DT, N_SUB = 5e-4, 50
THRESHOLDS = [(0.7, 1.5), (2.0, 1.5)]
CLASSES = [R.SETS["alpha"]["params"], R.SETS["wide"]["params"], R.DEFAULT]
_uniform = {}


def _class_runs(nsof_lib, ctx, torch_dev, grid, th, n_sub=N_SUB):
    """The three uniform device runs (one per class) on the frames of ``_array_case``: computed once per case, shared."""
    import torch
    key = (grid, th, n_sub)
    if key not in _uniform:
        imgs = _array_case(nsof_lib, ctx, grid, th)[0]
        d = torch.from_numpy(imgs.copy()).to(torch_dev)
        torch.cuda.synchronize(torch_dev)
        runs = []
        for p in CLASSES:
            out = nsof_lib.simulate_frames_dev(d, DT, n_sub, th[0], th[1], ctx=ctx, params=p)
            ctx.synchronize()
            runs.append(tuple(t.cpu().numpy() for t in out))
        for r in runs:
            for a in r:
                a.setflags(write=False)
        _uniform[key] = (imgs, d, runs)
    return _uniform[key]


def _labels(seed, shape):
    """A seeded class label per (trial, cell); all three classes occur wherever there are three cells."""
    n = int(np.prod(shape))
    return np.random.default_rng(seed).permutation(np.arange(n) % 3).reshape(shape)


def _class_planes(labels):
    """[T][H][W] float64 planes of all 13 keys: cell (t, r, c) is the device of class ``labels[t, r, c]``."""
    return {k: np.choose(labels, [float(p[k]) for p in CLASSES]) for k in R.KEYS}


def _by_class(labels, runs, which, per_frame):
    """``np.where`` over the class runs: output ``which`` (0 w, 1 res, 2 current) per (trial, cell)."""
    lab = labels[:, None] if per_frame else labels
    out = None
    for c, r in enumerate(runs):
        a = np.broadcast_to(r[which][None], (labels.shape[0],) + r[which].shape)
        out = np.where(lab == c, a, out if out is not None else a)
    return out


@pytest.mark.parametrize("trials", [1, 3])
@pytest.mark.parametrize("th", THRESHOLDS)
@pytest.mark.parametrize("grid", [(1, 1), (4, 4), (13, 24)])
def test_class_maps_equal_the_uniform_runs(nsof_lib, ctx, torch_dev, grid, th, trials):
    imgs, d, runs = _class_runs(nsof_lib, ctx, torch_dev, grid, th)
    for i in range(3):                                   # precondition: the three devices give three results
        for j in range(i):
            assert not np.array_equal(runs[i][0], runs[j][0]) and not np.array_equal(runs[i][1][1:], runs[j][1][1:])
    labels = _labels(grid[0] * 7 + trials, (trials,) + grid)
    if labels.size >= 3:
        assert np.unique(labels).size == 3
    w, res, cur = nsof_lib.simulate_frames_dev(d, DT, N_SUB, th[0], th[1], ctx=ctx, param_maps=_class_planes(labels))
    ctx.synchronize()
    assert w.shape == (trials,) + grid and res.shape == (trials, 5) + grid and cur.shape == (trials, 4) + grid
    assert np.array_equal(w.cpu().numpy(), _by_class(labels, runs, 0, False))
    assert np.array_equal(res.cpu().numpy(), _by_class(labels, runs, 1, True))
    assert np.array_equal(cur.cpu().numpy(), _by_class(labels, runs, 2, True))


def _cells_equal_the_host_entry(nsof_lib, ctx, imgs, th, got_w, got_res, params_at):
    """Every (trial, cell) of the mapped run equals the uniform HOST entry on that cell's 1 x 1 image stack."""
    trials, H, W = got_w.shape  # noqa: N806
    for t in range(trials):
        for r in range(H):
            for c in range(W):
                w1, res1 = nsof_lib.simulate_frames(imgs[:, r:r + 1, c:c + 1], DT, N_SUB, th[0], th[1], ctx=ctx,
                                                    params=params_at(t, r, c))
                assert got_w[t, r, c] == w1[0, 0], (t, r, c)
                assert np.array_equal(got_res[t, :, r, c], res1[:, 0, 0]), (t, r, c)


def test_random_spread_equals_the_uniform_entry_per_cell(nsof_lib, ctx, torch_dev):
    import torch
    from nsof.accumulator import variability_maps
    th = THRESHOLDS[0]
    imgs = _array_case(nsof_lib, ctx, (4, 4), th)[0]
    maps = variability_maps(4, 4, {k: 0.1 for k in R.KEYS}, None, seed=5, trials=3)
    assert all(maps[k].shape == (3, 4, 4) and maps[k].dtype == np.float32 and np.unique(maps[k]).size > 40 for k in R.KEYS)
    d = torch.from_numpy(imgs.copy()).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    w, res, cur = nsof_lib.simulate_frames_dev(d, DT, N_SUB, th[0], th[1], ctx=ctx, param_maps=maps)
    ctx.synchronize()
    w, res, cur = w.cpu().numpy(), res.cpu().numpy(), cur.cpu().numpy()
    assert np.isfinite(w).all() and np.isfinite(res).all()
    _cells_equal_the_host_entry(nsof_lib, ctx, imgs, th, w, res,
                                lambda t, r, c: dict(R.DEFAULT, **{k: float(maps[k][t, r, c]) for k in R.KEYS}))
    assert np.array_equal(cur, 1.0 / res[:, 1:])
    assert np.unique(w).size > 40                       # 48 devices, (nearly) as many results


def test_mixed_planes(nsof_lib, ctx, torch_dev):
    """One key shared by the trials ([H][W]), one per trial ([T][H][W]), the rest scalars of ``params``."""
    import torch
    th = THRESHOLDS[1]
    base = R.SETS["wide"]["params"]
    imgs = _array_case(nsof_lib, ctx, (4, 4), th)[0]
    rng = np.random.default_rng(8)
    koff = base["koff"] * (1 + 0.2 * rng.standard_normal((4, 4)))                      # float64, shared
    ron = (base["Ron"] * (1 + 0.1 * rng.standard_normal((2, 4, 4)))).astype(np.float32)   # float32, per trial
    d = torch.from_numpy(imgs.copy()).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    w, res, _ = nsof_lib.simulate_frames_dev(d, DT, N_SUB, th[0], th[1], ctx=ctx, params=base, param_maps=dict(koff=koff, Ron=ron))
    ctx.synchronize()
    w, res = w.cpu().numpy(), res.cpu().numpy()
    assert w.shape == (2, 4, 4) and not np.array_equal(res[0], res[1])
    _cells_equal_the_host_entry(nsof_lib, ctx, imgs, th, w, res,
                                lambda t, r, c: dict(base, koff=float(koff[r, c]), Ron=float(ron[t, r, c])))


@pytest.mark.parametrize("grid", [(1, 1), (4, 4), (13, 24)])
def test_constant_planes_give_the_uniform_bits(nsof_lib, ctx, torch_dev, grid):
    th = THRESHOLDS[0]
    imgs, d, runs = _class_runs(nsof_lib, ctx, torch_dev, grid, th)
    _, w_host, res_host = _array_case(nsof_lib, ctx, grid, th)          # the host entry, default device
    assert np.array_equal(runs[2][0], w_host) and np.array_equal(runs[2][1], res_host)
    for p, run in zip(CLASSES, runs):
        # 2-D constant planes of every key, next to scalars that are NOT the planes' values: the planes are what is read
        maps = {k: np.full(grid, float(p[k])) for k in R.KEYS}
        w, res, cur = nsof_lib.simulate_frames_dev(d, DT, N_SUB, th[0], th[1], ctx=ctx, params=CLASSES[1], param_maps=maps)
        ctx.synchronize()
        assert w.shape == (1,) + grid                   # a trial axis also for T = 1
        for got, want in zip((w, res, cur), run):
            assert np.array_equal(got[0].cpu().numpy(), want)
        # T identical trials give T identical results
        maps3 = {k: np.full((3,) + grid, float(p[k])) for k in R.KEYS}
        w3, res3, cur3 = nsof_lib.simulate_frames_dev(d, DT, N_SUB, th[0], th[1], ctx=ctx, param_maps=maps3)
        ctx.synchronize()
        for got, want in zip((w3, res3, cur3), run):
            g = got.cpu().numpy()
            assert all(np.array_equal(g[t], want) for t in range(3))
    # no planes, one trial: the _p_dev entry
    w0, res0, cur0 = nsof_lib.simulate_frames_dev(d, DT, N_SUB, th[0], th[1], ctx=ctx, params=CLASSES[0], param_maps={})
    ctx.synchronize()
    for got, want in zip((w0, res0, cur0), runs[0]):
        assert got.shape[0] == 1 and np.array_equal(got[0].cpu().numpy(), want)


@pytest.mark.parametrize("grid,n_sub,tol", [((4, 4), 10, 1e-12), ((13, 24), 10, 1e-12), ((4, 4), 1000, 1e-9)])
def test_against_the_restatement(nsof_lib, ctx, torch_dev, grid, n_sub, tol):
    """Bounds of test_accum_params_gpu.test_frame_driven_run_with_parameters: 1e-12 at n_sub 10, 1e-9 at n_sub 1000."""
    import torch
    th = THRESHOLDS[0]
    imgs = _array_case(nsof_lib, ctx, grid, th)[0]
    want = [R.simulate_frames(imgs, DT, n_sub, th[0], th[1], p=p) for p in CLASSES]
    labels = _labels(n_sub + grid[0], (2,) + grid)
    d = torch.from_numpy(imgs.copy()).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    w, res, _ = nsof_lib.simulate_frames_dev(d, DT, n_sub, th[0], th[1], ctx=ctx, param_maps=_class_planes(labels))
    ctx.synchronize()
    want_w = _by_class(labels, [(a, b) for a, b in want], 0, False).astype(np.float64)
    want_r = _by_class(labels, [(a, b) for a, b in want], 1, True).astype(np.float64)
    ew, er = np.abs(w.cpu().numpy() - want_w).max(), (np.abs(res.cpu().numpy() - want_r) / want_r).max()
    print(f"{grid} n_sub {n_sub}: max |w - restatement| {ew:.3g}, max rel res {er:.3g} (bound {tol:g})")
    assert ew <= tol and er <= tol


def _raw_dev(ctx, d_imgs, n, grid, th, v_ds, params, trials, maps, d_w, d_res, d_cur, n_sub=N_SUB, c_args=None):
    """nsof_accum_frames_f64_maps_dev called directly; ``maps`` = [(key, float64 [pt][H][W])]."""
    from nsof.accumulator import _frame_maps_c, accum_params
    ap = accum_params(params)
    keys, planes, counts = c_args if c_args is not None else _frame_maps_c(trials, maps)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    return ctx._lib.nsof_accum_frames_f64_maps_dev(ctx.ptr, ptr(d_imgs), n, grid[0], grid[1], DT, n_sub, th[0], th[1], v_ds,
                                                   C.byref(ap), trials, len(maps), keys, planes, counts, ptr(d_w), ptr(d_res),
                                                   ptr(d_cur))


@pytest.mark.parametrize("v_ds", [1.0, 0.5])
def test_entries_and_optional_outputs(nsof_lib, ctx, torch_dev, v_ds):
    import torch
    from nsof.accumulator import frame_param_maps_arg
    grid, th, T = (13, 24), THRESHOLDS[0], 3  # noqa: N806
    imgs, d, _ = _class_runs(nsof_lib, ctx, torch_dev, grid, th)
    labels = _labels(21, (T,) + grid)
    planes = _class_planes(labels)
    w, res, cur = nsof_lib.simulate_frames_dev(d, DT, N_SUB, th[0], th[1], v_ds, ctx=ctx, param_maps=planes)
    ctx.synchronize()
    w, res, cur = w.cpu().numpy(), res.cpu().numpy(), cur.cpu().numpy()
    assert np.array_equal(cur, v_ds / res[:, 1:])
    hw, hres = nsof_lib.simulate_frames(imgs, DT, N_SUB, th[0], th[1], ctx=ctx, param_maps=planes)     # the host entry
    assert hw.shape == w.shape and np.array_equal(hw, w) and np.array_equal(hres, res)
    # d_res NULL, d_current NULL: the other outputs keep their bits, the guards stay
    trials, maps = frame_param_maps_arg(planes, grid)
    for drop in ("res", "cur"):
        bw, tw = _guarded(torch, torch_dev, (T,) + grid)
        br, tr = _guarded(torch, torch_dev, (T, 5) + grid)
        bc, tc = _guarded(torch, torch_dev, (T, 4) + grid)
        torch.cuda.synchronize(torch_dev)
        rc = _raw_dev(ctx, d, 5, grid, th, v_ds, None, trials, maps, tw, None if drop == "res" else tr, None if drop == "cur" else tc)
        ctx.synchronize()
        assert rc == 0, ctx._lib.nsof_last_error(ctx.ptr)
        assert np.array_equal(tw.cpu().numpy(), w)
        assert (br.cpu().numpy() == SENTINEL).all() if drop == "res" else np.array_equal(tr.cpu().numpy(), res)
        assert (bc.cpu().numpy() == SENTINEL).all() if drop == "cur" else np.array_equal(tc.cpu().numpy(), cur)
        for b in (bw, br, bc):
            assert (b.cpu().numpy()[-GUARD:] == SENTINEL).all()


def test_one_frame_writes_the_initial_array_only(nsof_lib, ctx, torch_dev):
    import torch
    from nsof.accumulator import frame_param_maps_arg
    grid, th, T = (4, 4), THRESHOLDS[0], 2  # noqa: N806
    rng = np.random.default_rng(4)
    planes = dict(wini=rng.random((T,) + grid), Ron=163305.0 * (1 + 0.1 * rng.standard_normal(grid)),
                  Roff=2104377.0 * (1 + 0.1 * rng.standard_normal((T,) + grid)))
    trials, maps = frame_param_maps_arg(planes, grid)
    img = torch.from_numpy(rng.random((1,) + grid)).to(torch_dev)
    bw, tw = _guarded(torch, torch_dev, (T,) + grid)
    br, tr = _guarded(torch, torch_dev, (T, 1) + grid)
    bc, _ = _guarded(torch, torch_dev, (1,))
    torch.cuda.synchronize(torch_dev)
    assert _raw_dev(ctx, img, 1, grid, th, 1.0, None, trials, maps, tw, tr, bc[:1]) == 0
    ctx.synchronize()
    assert np.array_equal(tw.cpu().numpy(), planes["wini"])
    got = tr.cpu().numpy()
    for t in range(T):
        for r in range(4):
            for c in range(4):
                p = dict(R.DEFAULT, wini=planes["wini"][t, r, c], Ron=planes["Ron"][r, c], Roff=planes["Roff"][t, r, c])
                _, res1 = nsof_lib.simulate_frames(img[:, r:r + 1, c:c + 1].cpu().numpy(), ctx=ctx, params=p)
                assert got[t, 0, r, c] == res1[0, 0, 0], (t, r, c)       # the uniform entry's r0 of that cell
    assert (bc.cpu().numpy() == SENTINEL).all()                          # no current: nothing written
    assert (bw.cpu().numpy()[-GUARD:] == SENTINEL).all() and (br.cpu().numpy()[-GUARD:] == SENTINEL).all()


def test_refusals_leave_the_outputs_untouched(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import _lib
    from nsof.accumulator import _PARAM_KEYS
    grid, th, T = (4, 4), THRESHOLDS[0], 2  # noqa: N806
    d = torch.from_numpy(np.random.default_rng(0).random((3,) + grid)).to(torch_dev)
    bw, tw = _guarded(torch, torch_dev, (T,) + grid)
    br, tr = _guarded(torch, torch_dev, (T, 3) + grid)
    bc, tc = _guarded(torch, torch_dev, (T, 2) + grid)
    torch.cuda.synchronize(torch_dev)
    good = np.full((T,) + grid, 50.0)

    def status(trials=T, maps=(("koff", good),), c_args=None, params=None):
        rc = _raw_dev(ctx, d, 3, grid, th, 1.0, params, trials, list(maps), tw, tr, tc, c_args=c_args)
        return rc, (ctx._lib.nsof_last_error(ctx.ptr) or b"").decode()

    def c_arrays(keys, arrays, counts):
        return ((C.c_int * len(keys))(*keys), (C.c_void_p * len(keys))(*[None if a is None else a.ctypes.data for a in arrays]),
                (C.c_int * len(keys))(*counts))
    ikoff, ison = _PARAM_KEYS.index("koff"), _PARAM_KEYS.index("son")
    son = np.full((1,) + grid, 0.3)
    assert status(c_args=c_arrays([13], [good], [T]))[0] == _lib.NSOF_EINVAL                     # a key out of range
    assert status(c_args=c_arrays([-1], [good], [T]))[0] == _lib.NSOF_EINVAL
    rc, msg = status(maps=(("koff", good), ("koff", good)), c_args=c_arrays([ikoff, ikoff], [good, good], [T, T]))
    assert rc == _lib.NSOF_EINVAL and "twice" in msg                                                # a key given twice
    assert status(c_args=c_arrays([ikoff], [None], [T]))[0] == _lib.NSOF_EINVAL                  # a NULL plane
    for bad_count in (0, 3, -1):                                                                    # plane_trials not 1 or T
        assert status(c_args=c_arrays([ikoff], [good], [bad_count]))[0] == _lib.NSOF_EINVAL
    for bad_trials in (0, -2):                                                                      # n_trials < 1
        assert status(trials=bad_trials, maps=(("son", son),))[0] == _lib.NSOF_EINVAL
    assert status(maps=(("son", son),), params=dict(R.DEFAULT, voff=0.1))[0] == _lib.NSOF_EINVAL  # a bad scalar
    # one violation per rule of the domain, at trial 1, row 2, column 3
    rules = [("koff", np.nan), ("bon", np.inf), ("koff", 1e300), ("voff", 0.0), ("voff", 0.1), ("voff", -1e-60), ("von", 0.0),
             ("von", -0.1), ("son", 1.5), ("son", -0.1), ("soff", 1.0001), ("soff", -1e-9), ("wini", 1.5), ("wini", -0.1),
             ("Ron", 0.0), ("Ron", -5.0), ("Roff", 0.0), ("Roff", -1.0)]
    for key, bad in rules:
        plane = np.full((T,) + grid, float(R.DEFAULT[key]))
        plane[1, 2, 3] = bad
        rc, msg = status(maps=((key, plane),))
        assert rc == _lib.NSOF_EINVAL, (key, bad)
        assert key in msg and "trial 1" in msg and "row 2" in msg and "column 3" in msg, (key, bad, msg)
        if np.isfinite(bad):
            assert f"{bad:g}" in msg, (key, bad, msg)
    # ln(Roff / Ron) not finite: each value in its domain, their quotient underflows
    ron, roff = np.full((T,) + grid, 163305.0), np.full((1,) + grid, 2104377.0)
    ron[1, 2, 3], roff[0, 2, 3] = 1e30, 1e-300
    rc, msg = status(maps=(("Ron", ron), ("Roff", roff)))
    assert rc == _lib.NSOF_EINVAL and "trial 1" in msg and "row 2" in msg and "column 3" in msg, msg
    # a shared plane is checked as trial 0
    plane = np.full((1,) + grid, 0.3)
    plane[0, 0, 1] = 2.0
    rc, msg = status(maps=(("son", plane),))
    assert rc == _lib.NSOF_EINVAL and "trial 0" in msg and "row 0" in msg and "column 1" in msg
    # NULL frames or w; bad counts
    assert _raw_dev(ctx, None, 3, grid, th, 1.0, None, T, [("koff", good)], tw, tr, tc) == _lib.NSOF_EINVAL
    assert _raw_dev(ctx, d, 3, grid, th, 1.0, None, T, [("koff", good)], None, tr, tc) == _lib.NSOF_EINVAL
    assert _raw_dev(ctx, d, 0, grid, th, 1.0, None, T, [("koff", good)], tw, tr, tc) == _lib.NSOF_EINVAL
    assert _raw_dev(ctx, d, 3, grid, th, 1.0, None, T, [("koff", good)], tw, tr, tc, n_sub=0) == _lib.NSOF_EINVAL
    # from Python: shapes
    for bad_maps in (dict(koff=np.full((4, 5), 50.0)), dict(koff=good, son=np.full((3,) + grid, 0.3))):
        with pytest.raises(nsof_lib.error) as e:
            nsof_lib.simulate_frames_dev(d, ctx=ctx, param_maps=bad_maps)
        assert isinstance(e.value, ValueError) and e.value.status == _lib.NSOF_ESHAPE
    with pytest.raises(nsof_lib.error) as e:                       # the library's domain check reaches Python
        nsof_lib.simulate_frames_dev(d, ctx=ctx, param_maps=dict(von=np.full(grid, -0.5)))
    assert e.value.status == _lib.NSOF_EINVAL and "von" in str(e.value)
    ctx.synchronize()
    for b in (bw, br, bc):
        assert (b.cpu().numpy() == SENTINEL).all()                  # nothing was uploaded into, launched on or written
    # the host entry refuses the same way, its outputs untouched
    hw, hres = np.full((T,) + grid, SENTINEL), np.full((T, 3) + grid, SENTINEL)
    from nsof.accumulator import accum_params
    plane = np.full((T,) + grid, 0.1)
    plane[1, 2, 3] = -0.1
    keys, planes, counts = c_arrays([_PARAM_KEYS.index("von")], [plane], [T])
    himgs = d.cpu().numpy()
    rc = ctx._lib.nsof_accum_frames_f64_maps(ctx.ptr, himgs.ctypes.data, 3, 4, 4, DT, N_SUB, th[0], th[1],
                                             C.byref(accum_params(None)), T, 1, keys, planes, counts, hw.ctypes.data,
                                             hres.ctypes.data)
    assert rc == _lib.NSOF_EINVAL and (hw == SENTINEL).all() and (hres == SENTINEL).all()
    assert b"von" in ctx._lib.nsof_last_error(ctx.ptr)
