"""GPU: the accumulator with the device model, dt and refractory time as arguments.

Yardsticks: the goldens made by running the reference with non-default parameters (tests/golden/accum_params_*.npz) and the
NumPy restatement tests/accum_params_ref.py, whose contract -- float32 in the reference's order, every power and exp in
float64 from the float32 operands, rounded once -- is the device's.  The device's series are accurate to ~4e-14, so wherever
the restatement's long double evaluation says a power is farther than 2^-40 (relative) from a float32 rounding midpoint the
two must agree bit for bit; tests/test_accum_params_cpu.py checks that the simulate cases have no power closer than that.
Tolerances against the goldens: the reference's NumPy is 1-4 ulp off a correctly rounded float32 pow, hence the project's
1.2e-7 per step / W_ATOL per run / R_RTOL, widened by twice the measured reference-vs-restatement gap stored in the npz."""
import ctypes as C
import functools

import numpy as np
import pytest

import accum_params_ref as R
from conftest import golden_path, ulp_diff

pytestmark = pytest.mark.gpu

F = np.float32
W_ATOL = 5e-7
R_RTOL = 2e-6
NEAR = 2.0 ** -40
SIM = [(s, m) for s in R.SETS for m in R.MODES]


def stored_params(d):
    return dict(zip([str(k) for k in d["param_keys"]], [float(v) for v in d["param_values"]]))


@functools.lru_cache(maxsize=None)
def sim_case(name, mode):
    """(golden, restatement run) of one simulate golden; computed once, shared, never modified."""
    d = dict(np.load(golden_path(f"accum_params_sim_{name}_{mode}.npz")))
    H, W = d["w_final"].shape  # noqa: N806
    want = R.simulate(d["x"], d["y"], d["p"], d["t"], H, W, int(d["version"]), str(d["polarity"]), int(d["slice_us"]),
                      float(d["active_v"]), float(d["silent_v"]), stored_params(d), float(d["dt"]), int(d["refractory_us"]))
    return d, want


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaNs of any payload counting as equal."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return (a.view(np.int32) == b.view(np.int32)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name", list(R.SETS))
def test_update_state_and_resistance_with_parameters(nsof_lib, ctx, name):
    d = np.load(golden_path(f"accum_params_update_{name}.npz"))
    p, dt, gap = stored_params(d), float(d["dt"]), float(d["gap"])
    n = near = 0
    for wk, vk, ok in (("w_grid", "V_grid", "out_grid"), ("w_rand", "V_rand", "out_rand")):
        got = nsof_lib.update_state(d[wk], d[vk], p, dt, ctx=ctx)
        want, dist = R.update_state(d[wk], d[vk], p, dt, return_distance=True)
        assert got.dtype == F and got.shape == d[wk].shape
        eq, far = same_bits(got, want), dist >= NEAR
        print(f"{name} {wk}: {int((~eq).sum())} of {eq.size} differ from the restatement, {int((~far).sum())} near a midpoint, "
              f"max |got - golden| {np.nanmax(np.abs(got - d[ok])):.3g} (bound {2 * gap + 1.2e-7:.3g})")
        assert eq[far].all(), f"{wk}: differs from the restatement away from every rounding midpoint"
        assert (ulp_diff(got[~eq], want[~eq]) <= 1).all()
        n, near = n + eq.size, near + int((~far).sum())
        assert np.array_equal(np.isnan(got), np.isnan(d[ok]))
        assert np.nanmax(np.abs(got - d[ok])) <= 2 * gap + 1.2e-7
    assert near < 1e-3 * n
    for wk, rk in (("w_rand", "res_rand"), ("w_res", "res_grid")):
        r = nsof_lib.resistance_exp(d[wk], p, ctx=ctx)
        assert (np.abs(r - d[rk]) / d[rk]).max() <= R_RTOL
        assert (ulp_diff(r, R.resistance_exp(d[wk], p)) <= 1).all()
    # positional order of the reference, defaults = the fitted device
    w = d["w_rand"][:64]
    assert np.array_equal(nsof_lib.update_state(w, d["V_rand"][:64], ctx=ctx),
                          nsof_lib.update_state(w, d["V_rand"][:64], nsof_lib.PARAMS, nsof_lib.DT, ctx=ctx))
    assert np.array_equal(nsof_lib.resistance_exp(w, ctx=ctx), nsof_lib.resistance_exp(w, nsof_lib.PARAMS, ctx=ctx))


@pytest.mark.parametrize("name,mode", SIM)
def test_simulate_with_parameters(nsof_lib, ctx, name, mode):
    d, want = sim_case(name, mode)
    H, W = d["w_final"].shape  # noqa: N806
    out = nsof_lib.simulate((d["x"], d["y"], d["p"], d["t"]), version=int(d["version"]), slice_us=int(d["slice_us"]),
                            active_v=float(d["active_v"]), silent_v=float(d["silent_v"]), polarity=str(d["polarity"]),
                            sensor_size=(H, W), ctx=ctx, params=stored_params(d), dt=float(d["dt"]),
                            refractory_us=int(d["refractory_us"]))
    assert out["resistances"].shape[0] == int(d["n_snapshots"])
    idx = list(d["snap_idx"])
    tol = max(W_ATOL, 2 * float(d["gap"]))
    for k, rk in (("w_final", "resistances"), ("w_final_b", "resistances_b")):
        assert (k in out) == (k in d)
        if k not in d:
            continue
        print(f"{name} {mode} {k}: {int((~same_bits(out[k], want[k])).sum())} states differ from the restatement, "
              f"max |w - golden| {np.abs(out[k] - d[k]).max():.3g} (bound {tol:.3g})")
        assert same_bits(out[k], want[k]).all()
        assert (ulp_diff(out[rk], want[rk]) <= 1).all()
        assert np.abs(out[k] - d[k]).max() <= tol
        assert (np.abs(out[rk][idx] - d[rk]) / d[rk]).max() <= R_RTOL


def test_refractory_time_longer_than_two_slices(nsof_lib, ctx):
    """refractory_us = 1500 at 1000 us slices blocks the two slices after a pulse; the goldens' 20 / 45 us block the next
    slice only when its first event follows within that time."""
    d, _ = sim_case("alpha", "v2_split")
    H, W = d["w_final"].shape  # noqa: N806
    p, ev = stored_params(d), (d["x"], d["y"], d["p"], d["t"])
    outs = {}
    for refr in (1500, 0):
        out = nsof_lib.simulate(ev, version=2, active_v=-6.0, polarity="split", sensor_size=(H, W), ctx=ctx, params=p,
                                dt=float(d["dt"]), refractory_us=refr)
        want = R.simulate(*ev, H, W, 2, "split", 1000, -6.0, 0.0, p, float(d["dt"]), refr)
        assert same_bits(out["w_final"], want["w_final"]).all() and same_bits(out["w_final_b"], want["w_final_b"]).all()
        outs[refr] = out["w_final"]
    assert not np.array_equal(outs[1500], outs[0])


@pytest.mark.parametrize("name", list(R.SETS))
def test_every_update_form_with_parameters(nsof_lib, ctx, torch_dev, name):
    """One stream, a non-default device, through the every-pixel pass, the event-pixel update, run_surface and both forms of
    run_frames: the same states and the same 8-bit frames, the states of the restatement, the frames of the host map."""
    import torch
    from nsof.accumulator import Accumulator, slice_index_array
    d, _ = sim_case(name, "v1")
    cfg = R.SETS[name]
    H, W = d["w_final"].shape  # noqa: N806
    assert W == 64
    every, n_frames = 8, 6
    ev = (d["x"], d["y"], d["p"], d["t"])
    idx = slice_index_array(d["t"], 1000)
    model = dict(params=cfg["params"], dt=cfg["dt"], refractory_us=cfg["refractory_us"])
    states = [R.simulate(*ev, H, W, 1, "split", 1000, -6.0, 0.0, cfg["params"], cfg["dt"], n_slices=every * (k + 1))["w_final"]
              for k in range(n_frames)]
    assert len(np.unique(states[-1])) > 10
    for mode in ("state", "current"):
        host_frames = np.stack([R.surface_u8(s, cfg["params"], mode) for s in states])
        if mode == "state":   # (the current -> gray map saturates at 255 for these states, as it does for the fitted device)
            assert len(np.unique(host_frames)) > 5
        results = {}

        def run(label, how, **kw):
            acc = Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx, **model, **kw)
            frames = torch.zeros((n_frames, H, W), dtype=torch.uint8, device=torch_dev)
            try:
                acc.set_events(*ev, idx)
                how(acc, frames)
                ctx.synchronize()
                results[label] = (acc.w(0), frames.cpu().numpy())
            finally:
                acc.close()

        def per_interval(acc, frames):
            for k in range(n_frames):
                acc.run(k * every, every)
                acc.surface_u8(frames[k], mode=mode)

        def fused(acc, frames):
            for k in range(n_frames):
                acc.run_surface(k * every, every, frames[k], mode=mode)

        run("every-pixel pass", per_interval, dense=True)
        run("event-pixel update", per_interval, dense=False)
        run("run_surface", fused)
        run("run_frames tile walk", lambda acc, fr: acc.run_frames(0, n_frames, every, fr, mode=mode))
        run("run_frames copy + patch", lambda acc, fr: acc.run_frames(0, n_frames, every, fr, mode=mode), frames_path="copy_patch")
        for label, (w, frames) in results.items():
            assert same_bits(w, states[-1]).all(), (mode, label)
            assert np.array_equal(frames, host_frames), (mode, label, int((frames != host_frames).sum()))


def test_silent_voltage_inside_a_wider_dead_zone(nsof_lib, ctx, oracle):
    """silent_v = 0.2 lies inside [voff, von] = [-0.6, 0.25]: idle pixels keep their bits and the event-pixel update is exact;
    the fitted device (von = 0.1) leaks at the same voltage."""
    d, _ = sim_case("wide", "v1")
    cfg = R.SETS["wide"]
    H, W = d["w_final"].shape  # noqa: N806
    ev = (d["x"], d["y"], d["p"], d["t"])
    kw = dict(version=1, active_v=-6.0, silent_v=0.2, sensor_size=(H, W), ctx=ctx)
    model = dict(params=cfg["params"], dt=cfg["dt"])
    touched = np.zeros((H, W), bool)
    touched[d["y"], d["x"]] = True
    sparse = nsof_lib.simulate(ev, dense=False, **kw, **model)["w_final"]
    dense = nsof_lib.simulate(ev, dense=True, **kw, **model)["w_final"]
    auto = nsof_lib.simulate(ev, **kw, **model)["w_final"]
    want = R.simulate(*ev, H, W, 1, "split", 1000, -6.0, 0.2, cfg["params"], cfg["dt"])["w_final"]
    assert (~touched).sum() > 1000 and (sparse[~touched].view(np.int32) == F(cfg["params"]["wini"]).view(np.int32)).all()
    assert np.array_equal(sparse, dense) and np.array_equal(sparse, auto) and same_bits(sparse, want).all()
    leak = nsof_lib.simulate(ev, **kw)["w_final"]
    ref = oracle.accum_simulate(*ev, H, W, 1, "split", 1000, -6.0, 0.2)["w_final"]
    assert (leak[~touched] < 0.5).all() and np.abs(leak - ref).max() <= W_ATOL


def test_three_devices_on_one_context(nsof_lib, ctx, oracle):
    """Two accumulators with different parameters and a default one, stepped alternately on one context: each equals its own
    uninterrupted run, the default one the C oracle (correctly rounded mode, outside its device band)."""
    from nsof.accumulator import Accumulator, slice_index_array
    d, _ = sim_case("alpha", "v2_split")
    H, W = d["w_final"].shape  # noqa: N806
    ev = (d["x"], d["y"], d["p"], d["t"])
    idx = slice_index_array(d["t"], 1000)
    n = len(idx) - 1
    models = {"alpha": dict(params=R.SETS["alpha"]["params"], dt=R.SETS["alpha"]["dt"], refractory_us=20),
              "wide": dict(params=R.SETS["wide"]["params"], dt=R.SETS["wide"]["dt"], refractory_us=45), "default": {}}
    accs = {k: Accumulator(H, W, 2, "split", -6.0, 0.0, ctx=ctx, **m) for k, m in models.items()}
    try:
        for a in accs.values():
            a.set_events(*ev, idx)
        for lo in range(0, n, 23):
            for a in accs.values():
                a.run(lo, min(23, n - lo))
        got = {k: (a.w(0), a.w(1)) for k, a in accs.items()}
        assert accs["alpha"].params["alphaoff"] == 1.5 and accs["wide"].refractory_us == 45 and accs["default"].dt == 5e-4
    finally:
        for a in accs.values():
            a.close()
    for k, m in models.items():
        one = nsof_lib.simulate(ev, version=2, active_v=-6.0, polarity="split", sensor_size=(H, W), ctx=ctx, **m)
        assert np.array_equal(got[k][0], one["w_final"]) and np.array_equal(got[k][1], one["w_final_b"]), k
    assert not np.array_equal(got["alpha"][0], got["wide"][0]) and not np.array_equal(got["alpha"][0], got["default"][0])
    ref = oracle.accum_simulate(*ev, H, W, 2, "split", 1000, -6.0, 0.0, rounding="correct")
    for w, wk, bk in ((got["default"][0], "w_final", "band_px"), (got["default"][1], "w_final_b", "band_px_b")):
        assert np.array_equal(w[~ref[bk]], ref[wk][~ref[bk]]) and np.abs(w - ref[wk]).max() <= W_ATOL


def test_frame_driven_run_with_parameters(nsof_lib, ctx, torch_dev):
    import torch
    p = R.SETS["alpha"]["params"]
    rng = np.random.default_rng(3)
    for shape in ((4, 4), (9, 31)):
        imgs = rng.random((5,) + shape)
        for n_sub, tol in ((1000, 1e-9), (10, 1e-12)):
            want_w, want_r = R.simulate_frames(imgs, n_sub=n_sub, p=p)
            w, res = nsof_lib.simulate_frames(imgs, n_sub_steps=n_sub, ctx=ctx, params=p)
            print(f"{shape} n_sub {n_sub}: max |w - restatement| {np.abs(w - want_w).max():.3g} (bound {tol:g})")
            assert np.abs(w - want_w).max() <= tol and (np.abs(res - want_r) / want_r).max() <= tol
            dw, dres, dcur = nsof_lib.simulate_frames_dev(torch.from_numpy(imgs).to(torch_dev), n_sub_steps=n_sub, v_ds=0.7,
                                                          ctx=ctx, params=p)
            ctx.synchronize()
            assert np.array_equal(dw.cpu().numpy(), w) and np.array_equal(dres.cpu().numpy(), res)
            assert np.array_equal(dcur.cpu().numpy(), 0.7 / res[1:])
        w0, _ = nsof_lib.simulate_frames(imgs, ctx=ctx)
        assert np.abs(w0 - w).max() > 1e-3      # the parameters reach the kernel


BAD = [(k, v) for k in R.KEYS for v in (np.nan, np.inf)] + [
    ("voff", 0.0), ("voff", 0.1), ("von", 0.0), ("von", -0.1), ("voff", -1e-60), ("son", 1.5), ("son", -0.1), ("soff", 1.0001),
    ("soff", -1e-9), ("Ron", 0.0), ("Ron", -5.0), ("Roff", 0.0), ("Roff", -1.0), ("wini", 1.5), ("wini", -0.1), ("koff", 1e300)]


def test_invalid_parameters_are_refused_before_any_launch(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import _lib
    from nsof.accumulator import Accumulator, accum_params
    from nsof.context import dev_ptr
    lib = ctx._lib
    w = torch.full((256,), 0.5, dtype=torch.float32, device=torch_dev)
    V = torch.full((256,), -6.0, dtype=torch.float32, device=torch_dev)  # noqa: N806
    out = torch.full((256,), -7.0, dtype=torch.float32, device=torch_dev)
    imgs = np.random.default_rng(0).random((3, 4, 4))
    d_imgs = torch.from_numpy(imgs).to(torch_dev)
    cases = [dict(params=dict(nsof_lib.PARAMS, **{k: v})) for k, v in BAD]
    cases += [dict(dt=v) for v in (0.0, -1e-4, np.nan, np.inf, 1e-60)] + [dict(refractory_us=-1)]
    for model in cases:
        ap = accum_params(**model)
        with pytest.raises(nsof_lib.error) as e:
            Accumulator(8, 8, 2, "split", -6.0, 0.0, ctx=ctx, **model)
        assert e.value.status == _lib.NSOF_EINVAL, model
        p = C.c_void_p()
        assert lib.nsof_accum_create_p(ctx.ptr, 8, 8, 1, 0, -6.0, 0.0, C.byref(ap), C.byref(p)) == _lib.NSOF_EINVAL and not p.value
        assert lib.nsof_accum_update_state_p_dev(ctx.ptr, C.byref(ap), dev_ptr(w), dev_ptr(V), dev_ptr(out), 256) == _lib.NSOF_EINVAL
        assert lib.nsof_accum_resistance_p_dev(ctx.ptr, C.byref(ap), dev_ptr(w), dev_ptr(out), 256) == _lib.NSOF_EINVAL
        hw, hres = np.full((4, 4), -7.0), np.full((3, 4, 4), -7.0)
        assert lib.nsof_accum_frames_f64_p(ctx.ptr, imgs.ctypes.data, 3, 4, 4, 5e-4, 10, 0.7, 1.5, C.byref(ap), hw.ctypes.data,
                                           hres.ctypes.data) == _lib.NSOF_EINVAL
        assert (hw == -7.0).all() and (hres == -7.0).all()
        dw = torch.full((4, 4), -7.0, dtype=torch.float64, device=torch_dev)
        dres = torch.full((3, 4, 4), -7.0, dtype=torch.float64, device=torch_dev)
        assert lib.nsof_accum_frames_f64_p_dev(ctx.ptr, dev_ptr(d_imgs), 3, 4, 4, 5e-4, 10, 0.7, 1.5, 1.0, C.byref(ap), dev_ptr(dw),
                                               dev_ptr(dres), None) == _lib.NSOF_EINVAL
        ctx.synchronize()
        assert bool((dw == -7.0).all()) and bool((dres == -7.0).all())
    ctx.synchronize()
    assert bool((out == -7.0).all())
    for fn in (lambda m: nsof_lib.update_state(np.zeros(4, F), np.zeros(4, F), m["params"], ctx=ctx),
               lambda m: nsof_lib.resistance_exp(np.zeros(4, F), m["params"], ctx=ctx),
               lambda m: nsof_lib.simulate_frames(imgs, ctx=ctx, params=m["params"]),
               lambda m: nsof_lib.simulate_frames_dev(d_imgs, ctx=ctx, params=m["params"])):
        with pytest.raises(nsof_lib.error):
            fn(cases[0])
    with pytest.raises(nsof_lib.error, match="'bon'"):
        nsof_lib.update_state(np.zeros(4, F), np.zeros(4, F), {k: v for k, v in nsof_lib.PARAMS.items() if k != "bon"}, ctx=ctx)
    with pytest.raises(nsof_lib.error, match="'Roff'"):
        Accumulator(8, 8, ctx=ctx, params={k: v for k, v in nsof_lib.PARAMS.items() if k != "Roff"})
    # the limits themselves are accepted
    ok = dict(nsof_lib.PARAMS, son=0.0, soff=1.0, wini=0.0)
    acc = Accumulator(8, 8, ctx=ctx, params=ok, refractory_us=0)
    assert acc.params["soff"] == 1.0 and (acc.w(0) == 0).all()
    acc.close()


def test_band_factory_on_a_group_of_one_rank(nsof_lib, ctx):
    """nsof.dist.accumulator_band as the callback of simulate_banded (RCCL, one rank) with a non-default device, scheme 2 /
    split: the gathered bands equal the unsharded simulate bit for bit."""
    import os

    import torch.distributed as dist
    from nsof import dist as nd
    d, _ = sim_case("wide", "v2_split")
    cfg = R.SETS["wide"]
    H, W = d["w_final"].shape  # noqa: N806
    ev = (d["x"], d["y"], d["p"], d["t"])
    model = dict(params=cfg["params"], dt=cfg["dt"], refractory_us=cfg["refractory_us"])
    one = nsof_lib.simulate(ev, version=2, active_v=-6.0, polarity="split", sensor_size=(H, W), ctx=ctx, **model)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(29910 + os.getpid() % 40)
    for k, v in (("RANK", "0"), ("WORLD_SIZE", "1"), ("LOCAL_RANK", "0")):
        os.environ.setdefault(k, v)
    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl")
    try:
        wa, wb = nd.simulate_banded(*ev, (H, W), 1000, nd.accumulator_band(2, "split", -6.0, 0.0, ctx=ctx, **model))
    finally:
        if created:
            dist.destroy_process_group()
    assert np.array_equal(wa.numpy(), one["w_final"]) and np.array_equal(wb.numpy(), one["w_final_b"])
    assert not np.array_equal(wa.numpy(), nsof_lib.simulate(ev, version=2, active_v=-6.0, polarity="split", sensor_size=(H, W),
                                                            ctx=ctx)["w_final"])
