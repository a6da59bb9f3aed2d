"""GPU: the arithmetic of the frame-driven array run, pinned bit for bit to ``tests/golden/frames_run_bits.npz`` -- the
``w`` and ``res`` that the per-pair host entry returned (one ``k_frame_step`` launch per frame pair, the oldest statement
of the contract; that entry is gone, ``scripts/make_frames_bits_golden.py`` wrote its results down first).  Every way into
the one kernel must give those bits: both Python functions, the four uniform entries of the C ABI, the mapped entries
without maps, with constant planes equal to the scalars (``kon``, ``Ron``, ``wini``: so the host-formed ``lambda`` and
``r0`` planes are read too), and with three identical trials.  (The check of the fixture itself needs no GPU.)"""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

import accum_params_ref as R

DT, N_SUB, V_DS = 5e-4, 50, 0.5
DEVICES = {"default": None, "alpha": R.SETS["alpha"]["params"], "wide": R.SETS["wide"]["params"]}
_GOLDEN = np.load(Path(__file__).parent / "golden" / "frames_run_bits.npz")
CASES = json.loads(str(_GOLDEN["cases"]))


def _inputs(case):
    grid = tuple(case["grid"])
    imgs = _GOLDEN[f"imgs_{grid[0]}x{grid[1]}"][:case["n_frames"]]
    return grid, imgs, _GOLDEN[f"w_{case['name']}"], _GOLDEN[f"res_{case['name']}"]


def _regimes(imgs, th1, voff, von):
    d = np.abs(imgs[:-1] * 256 - imgs[1:] * 256)
    v = np.where(d > th1, (d + 4) * 0.75, (d - 5.5) * 0.6)
    v = np.where(v > 0, -(0.3 * v + 0), np.where(v < 0, -(3 * v + -3), 0.0))
    return int((v < voff).sum()), int((v > von).sum()), int(((v >= voff) & (v <= von)).sum())


def test_fixture_reaches_every_regime():
    """What the generator asserted, on the stored frames: a regenerated fixture cannot quietly lose the dead-zone cells."""
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names) == 30
    assert {(c["device"], tuple(c["grid"])) for c in CASES} == (
        {("default", g) for g in [(1, 1), (4, 4), (6, 8), (13, 24)]} | {(d, g) for d in ("alpha", "wide") for g in [(4, 4), (13, 24)]})
    assert {(c["th1"], c["th2"]) for c in CASES} == {(0.7, 1.5), (2.0, 1.5), (8.0, 1.5)}
    assert {c["n_frames"] for c in CASES if c["device"] == "default" and c["grid"] == [4, 4]} == {1, 2, 5}
    dead_cases = 0
    for c in CASES:
        grid, imgs, w, res = _inputs(c)
        assert imgs.shape == (c["n_frames"],) + grid and w.shape == grid and res.shape == imgs.shape
        if c["n_frames"] > 1:                         # one frame: res is r0 alone
            assert np.unique(res).size > 2, c["name"]
        if c["n_frames"] < 5:
            continue
        p = DEVICES[c["device"]] or R.DEFAULT
        counts = _regimes(imgs, c["th1"], p["voff"], p["von"])
        if c["th1"] == 8.0 and grid[0] >= 4:
            assert min(counts) > 0, (c["name"], counts)
            dead_cases += 1
    assert dead_cases == 7
    assert _regimes(_GOLDEN["imgs_13x24"], 8.0, -0.2, 0.1) == (459, 774, 15)


def _maps_dev_raw(ctx, d_imgs, case, n_trials):
    """``nsof_accum_frames_f64_maps_dev`` with no maps and ``n_trials`` trials, through ctypes."""
    import torch
    from nsof.accumulator import accum_params
    from nsof.context import dev_ptr
    n, H, W = d_imgs.shape  # noqa: N806
    w = torch.empty((n_trials, H, W), dtype=torch.float64, device=d_imgs.device)
    res = torch.empty((n_trials, n, H, W), dtype=torch.float64, device=d_imgs.device)
    cur = torch.empty((n_trials, n - 1, H, W), dtype=torch.float64, device=d_imgs.device)
    ap = accum_params(DEVICES[case["device"]])
    rc = ctx._lib.nsof_accum_frames_f64_maps_dev(ctx.ptr, dev_ptr(d_imgs), n, H, W, DT, N_SUB, case["th1"], case["th2"], V_DS,
                                                 C.byref(ap), n_trials, 0, None, None, None, dev_ptr(w), dev_ptr(res),
                                                 dev_ptr(cur) if n > 1 else None)
    assert rc == 0, ctx._lib.nsof_last_error(ctx.ptr)
    return w, res, cur


def _uniform_raw(ctx, imgs, d_imgs, case, ap):
    """The four uniform entries of the C ABI through ctypes -- ``nsof_accum_frames_f64`` / ``_dev`` where ``ap`` is None,
    ``_p`` / ``_p_dev`` with ``ap`` (an ``AccumParams``, or None for NULL params): ``(w, res)`` of the host entry and
    ``(w, res, current)`` of the device entry, as NumPy arrays."""
    import torch
    from nsof.context import dev_ptr
    lib = ctx._lib
    n, H, W = imgs.shape  # noqa: N806
    sizes = (n, H, W, DT, N_SUB, case["th1"], case["th2"])
    w, res = np.empty((H, W)), np.empty((n, H, W))
    dw, dres, dcur = (torch.empty(s, dtype=torch.float64, device=d_imgs.device) for s in ((H, W), (n, H, W), (n - 1, H, W)))
    cur = dev_ptr(dcur) if n > 1 else None
    if ap is None:
        rc_h = lib.nsof_accum_frames_f64(ctx.ptr, imgs.ctypes.data, *sizes, w.ctypes.data, res.ctypes.data)
        rc_d = lib.nsof_accum_frames_f64_dev(ctx.ptr, dev_ptr(d_imgs), *sizes, V_DS, dev_ptr(dw), dev_ptr(dres), cur)
    else:
        par = C.byref(ap) if ap != "null" else None
        rc_h = lib.nsof_accum_frames_f64_p(ctx.ptr, imgs.ctypes.data, *sizes, par, w.ctypes.data, res.ctypes.data)
        rc_d = lib.nsof_accum_frames_f64_p_dev(ctx.ptr, dev_ptr(d_imgs), *sizes, V_DS, par, dev_ptr(dw), dev_ptr(dres), cur)
    assert rc_h == 0 and rc_d == 0, lib.nsof_last_error(ctx.ptr)
    ctx.synchronize()
    return (w, res), tuple(t.cpu().numpy() for t in (dw, dres, dcur))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_every_entry_gives_the_recorded_bits(nsof_lib, ctx, torch_dev, case):
    import torch
    grid, imgs, w_ref, res_ref = _inputs(case)
    params = DEVICES[case["device"]]
    p = params or R.DEFAULT
    const = {k: np.full(grid, float(p[k])) for k in ("kon", "Ron", "wini")}
    args = (DT, N_SUB, case["th1"], case["th2"])
    d = torch.from_numpy(imgs.copy()).to(torch_dev)
    torch.cuda.synchronize(torch_dev)

    def host(trials, got):
        w, res = got
        assert w.shape == trials + grid and res.shape == trials + res_ref.shape
        for t in range(trials[0] if trials else 1):
            assert np.array_equal(w[t] if trials else w, w_ref) and np.array_equal(res[t] if trials else res, res_ref)

    def dev(trials, got):
        ctx.synchronize()
        w, res, cur = (t.cpu().numpy() for t in got)
        host(trials, (w, res))
        assert cur.shape == trials + (case["n_frames"] - 1,) + grid
        assert np.array_equal(cur, V_DS / res[..., 1:, :, :])

    host((), nsof_lib.simulate_frames(imgs, *args, ctx=ctx, params=params))
    dev((), nsof_lib.simulate_frames_dev(d, *args, V_DS, ctx=ctx, params=params))
    host((1,), nsof_lib.simulate_frames(imgs, *args, ctx=ctx, params=params, param_maps={}))       # the maps entries, no maps
    dev((1,), nsof_lib.simulate_frames_dev(d, *args, V_DS, ctx=ctx, params=params, param_maps={}))
    host((1,), nsof_lib.simulate_frames(imgs, *args, ctx=ctx, params=params, param_maps=const))    # constant planes
    dev((1,), nsof_lib.simulate_frames_dev(d, *args, V_DS, ctx=ctx, params=params, param_maps=const))
    dev((3,), _maps_dev_raw(ctx, d, case, 3))                                                      # three identical trials
    # the uniform entries of the C ABI themselves (the Python functions above go through the maps entries): without a
    # params argument and with NULL params on the default device, with the explicit set on every device
    from nsof.accumulator import accum_params
    for ap in ([None, "null"] if params is None else []) + [accum_params(params)]:
        got_host, got_dev = _uniform_raw(ctx, np.ascontiguousarray(imgs), d, case, ap)
        host((), got_host)
        w, res, cur = got_dev
        host((), (w, res))
        assert cur.shape == (case["n_frames"] - 1,) + grid and np.array_equal(cur, V_DS / res[1:])
