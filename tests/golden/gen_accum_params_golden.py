#!/opt/conda/bin/python3.9
"""Golden vectors for the accumulator with NON-DEFAULT device parameters, made by RUNNING THE REFERENCE ITSELF.

Run in the build container only (the reference never travels):
    /opt/conda/bin/python3.9 tests/golden/gen_accum_params_golden.py
Imports /root/reference/eventsim/event_mem_sim.py (numpy 1.26.4, h5py 3.3.0; `cv2` stubbed as in gen_accum_golden.py)
and runs it with altered parameters the way the reference allows: ``update_state(w, V, p, dt)`` / ``resistance_exp(w, p)``
directly, and ``simulate`` after mutating ``PARAMS`` in place, setting ``REFRACTORY_US`` and replacing
``update_state.__defaults__`` (dt).  Writes tests/golden/accum_params_update_<set>.npz and
tests/golden/accum_params_sim_<set>_<mode>.npz: the inputs, the parameter set and the reference's outputs, plus `gap`, the
measured maximum difference between the reference and the restatement tests/accum_params_ref.py (the tests' tolerance
against these files is built on it).

Every stream's seed is searched, with the restatement alone, until the run's closest approach of a power to a float32
rounding midpoint (long double evaluation) exceeds 2^-40 relative: only then must the device equal the restatement bit for
bit.  Checked here as well: fewer than 1 % of a simulate golden's final states equal 0 or 1 and at least 100 distinct
state values occur (a device whose states run into the clip tests nothing).
"""
import sys
import tempfile
import types
from pathlib import Path

sys.modules["cv2"] = types.ModuleType("cv2")
sys.path.insert(0, "/root/reference/eventsim")
OUT = Path(__file__).resolve().parent
sys.path.insert(0, str(OUT.parent))
import h5py  # noqa: E402
import numpy as np  # noqa: E402
import event_mem_sim as ems  # noqa: E402
import accum_params_ref as R  # noqa: E402

F = np.float32
NEAR = 2.0 ** -40
W, H, N_EVENTS, N_SLICES, SLICE_US = 64, 48, 6000, 200, 1000
RAMP, PROBES, RUN = 100, 40, 20


def make_stream(seed):
    """Without a leak a pixel's final state is a function of its number of pulses alone, so distinct states need distinct
    pulse counts: RAMP pixels at random places (the sensor's last pixel among them: the loader infers the size from the
    largest coordinate), pixel j with events in j distinct EVEN slices -- never two consecutive ones, so a refractory time
    below one slice blocks none of them -- with polarity 0 for j <= 30 (array B of scheme 2 / split) and 1 above.  The
    refractory rule is probed by PROBES further pixels with an event in each of RUN consecutive slices, random polarity:
    whether slice s + 1 is blocked depends on the gap between the last event of slice s and the first of slice s + 1.  The
    events left are duplicates of existing (pixel, slice) pairs.  Times are uniform inside their slice; sorted by time as
    the reference expects."""
    rng = np.random.default_rng(seed)
    where = rng.choice(W * H - 1, RAMP + PROBES - 1, replace=False)
    where = np.append(where, W * H - 1)[::-1]
    xs, ys, ps, sl = [], [], [], []
    for j, px in enumerate(where[:RAMP], start=1):
        s = 2 * rng.choice(N_SLICES // 2, j, replace=False)
        xs.append(np.full(j, px % W)); ys.append(np.full(j, px // W)); ps.append(np.full(j, 0 if j <= 30 else 1)); sl.append(s)
    for px in where[RAMP:]:
        s = rng.integers(0, N_SLICES - RUN) + np.arange(RUN)
        xs.append(np.full(RUN, px % W)); ys.append(np.full(RUN, px // W)); ps.append(rng.integers(0, 2, RUN)); sl.append(s)
    x, y, p, sl = (np.concatenate(a) for a in (xs, ys, ps, sl))
    extra = rng.integers(0, x.size, N_EVENTS - x.size)
    x, y, sl = np.append(x, x[extra]), np.append(y, y[extra]), np.append(sl, sl[extra])
    p = np.append(p, rng.integers(0, 2, extra.size))
    t = sl * SLICE_US + rng.integers(0, SLICE_US, x.size)
    t[np.argmin(t)] = 0                          # the slice grid starts at the first event
    order = np.argsort(t, kind="stable")
    return x[order].astype(np.int16), y[order].astype(np.int16), p[order].astype(np.int8), t[order].astype(np.int64)


def param_arrays(cfg):
    p = cfg["params"]
    return dict(param_keys=np.array(list(p)), param_values=np.array([float(p[k]) for k in p], np.float64),
                dt=np.float64(cfg["dt"]), refractory_us=np.int64(cfg["refractory_us"]))


def update_grid(p):
    """The clip, the thresholds voff / von and their float32 neighbours, and states outside [0, 1] (negative and zero bases
    of the power, with the set's integer and non-integer exponents)."""
    voff, von = F(p["voff"]), F(p["von"])
    lo, hi = F(-np.inf), F(np.inf)
    V = np.array([-8, -6, -1, np.nextafter(voff, lo), voff, np.nextafter(voff, hi), 0, np.nextafter(von, lo), von,  # noqa: N806
                  np.nextafter(von, hi), 0.5, 1, 3, 6], F)
    w = np.array([-2.5, -0.5, 0, 1e-6, 0.01, 0.25, 0.5, 0.75, 0.99, 0.999999, 1, 1 / 0.7, 1.5, 3, 5, 1 / 0.3], F)
    Vg, wg = np.meshgrid(V, w, indexing="ij")  # noqa: N806
    return np.ascontiguousarray(wg, F), np.ascontiguousarray(Vg, F)


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def gen_update(name, cfg):
    p, dt = cfg["params"], cfg["dt"]
    wg, Vg = update_grid(p)  # noqa: N806
    with np.errstate(all="ignore"):
        out_grid = np.asarray(ems.update_state(wg, Vg, p, dt), F)
    for seed in range(100, 200):
        rng = np.random.default_rng(seed)
        wr = rng.random(4096, dtype=F)
        Vr = (rng.random(4096, dtype=F) * 16 - 8).astype(F)  # noqa: N806
        mine, dist = R.update_state(wr, Vr, p, dt, return_distance=True)
        _, dist_g = R.update_state(wg, Vg, p, dt, return_distance=True)
        if (dist < NEAR).sum() + (dist_g < NEAR).sum() == 0:
            break
    else:
        raise SystemExit("no seed without a near-midpoint power")
    out_rand = np.asarray(ems.update_state(wr, Vr, p, dt), F)
    res_rand = np.asarray(ems.resistance_exp(wr, p), F)
    res_grid = np.asarray(ems.resistance_exp(wg[0], p), F)
    mine_g = R.update_state(wg, Vg, p, dt)
    assert same_nan(mine_g, out_grid), "nan pattern of the grid differs"
    gap = max(float(np.nanmax(np.abs(mine_g - out_grid))), float(np.abs(mine - out_rand).max()))
    rgap = max(float((np.abs(R.resistance_exp(wr, p) - res_rand) / res_rand).max()),
               float(np.nanmax(np.abs(R.resistance_exp(wg[0], p) - res_grid) / res_grid)))
    np.savez_compressed(OUT / f"accum_params_update_{name}.npz", w_grid=wg, V_grid=Vg, out_grid=out_grid, w_rand=wr, V_rand=Vr,
                        out_rand=out_rand, res_rand=res_rand, w_res=wg[0], res_grid=res_grid, seed=seed, gap=np.float64(gap),
                        res_gap=np.float64(rgap), **param_arrays(cfg))
    print(f"update {name}: seed {seed}, gap {gap:.3g}, resistance gap {rgap:.3g} (relative), nan in grid {int(np.isnan(out_grid).sum())}")


def run_reference(stream, cfg, version, polarity, active_v, silent_v, keep=(0, 1, -1)):
    x, y, p, t = stream
    saved = dict(ems.PARAMS), ems.REFRACTORY_US, ems.update_state.__defaults__
    try:
        ems.PARAMS.update(cfg["params"])                                  # in place: update_state's default p is this dict
        ems.REFRACTORY_US = cfg["refractory_us"]
        ems.update_state.__defaults__ = (ems.PARAMS, cfg["dt"])
        with tempfile.TemporaryDirectory() as d:
            h5 = Path(d) / "s.hdf5"
            with h5py.File(h5, "w") as f:
                g = f.create_group("/CD/events")
                for k, v, ty in (("x", x, np.int16), ("y", y, np.int16), ("p", p, np.int8), ("t", t, np.int64)):
                    g.create_dataset(k, data=v, dtype=ty)
            ems.simulate(h5, version=version, slice_us=SLICE_US, active_v=active_v, silent_v=silent_v, save_video=False,
                         polarity=polarity)
            a = np.load(h5.with_suffix(f".V{version}.npz"))
            out = dict(w_final=a["w_final"], n_snapshots=a["resistances"].shape[0], snap_idx=np.array(keep),
                       resistances=a["resistances"][list(keep)])
            if version == 2 and polarity == "split":
                b = np.load(h5.with_suffix(".V2_b.npz"))
                out.update(w_final_b=b["w_final"], resistances_b=b["resistances"][list(keep)])
    finally:
        ems.PARAMS.clear()
        ems.PARAMS.update(saved[0])
        ems.REFRACTORY_US = saved[1]
        ems.update_state.__defaults__ = saved[2]
    return out


def gen_sim(name, cfg, mode, first_seed):
    version, polarity, sil = R.MODES[mode]
    silent_v = cfg["leak_v"] if sil == "leak" else 0.0
    active_v = cfg["active_v"]
    for seed in range(first_seed, first_seed + 200):
        stream = make_stream(seed)
        mid = R.Midpoints()
        mine = R.simulate(*stream, H, W, version, polarity, SLICE_US, active_v, silent_v, cfg["params"], cfg["dt"],
                          cfg["refractory_us"], mid=mid)
        finals = np.concatenate([mine[k].ravel() for k in ("w_final", "w_final_b") if k in mine])
        if mid.closest > NEAR and len(np.unique(finals)) >= 100:
            break
    else:
        raise SystemExit(f"{name} {mode}: no seed with a closest midpoint approach above 2^-40 and 100 distinct final states")
    ref = run_reference(stream, cfg, version, polarity, active_v, silent_v)
    gap, rgap = 0.0, 0.0
    finals = np.concatenate([ref[k].ravel() for k in ("w_final", "w_final_b") if k in ref])   # both arrays of a split run
    clipped, distinct = float(((finals == 0) | (finals == 1)).mean()), len(np.unique(finals))
    assert clipped < 0.01 and distinct >= 100, f"{name} {mode}: {clipped:.3%} clipped, {distinct} distinct states"
    for k in ("w_final", "w_final_b"):
        if k in ref:
            gap = max(gap, float(np.abs(mine[k] - ref[k]).max()))
    for k in ("resistances", "resistances_b"):
        if k in ref:
            rgap = max(rgap, float((np.abs(mine[k][list(ref["snap_idx"])] - ref[k]) / ref[k]).max()))
    assert mine["resistances"].shape[0] == ref["n_snapshots"]
    x, y, p, t = stream
    np.savez_compressed(OUT / f"accum_params_sim_{name}_{mode}.npz", x=x, y=y, p=p, t=t, version=version, polarity=polarity,
                        slice_us=SLICE_US, active_v=F(active_v), silent_v=F(silent_v), seed=seed, gap=np.float64(gap),
                        res_gap=np.float64(rgap), closest_midpoint=np.float64(mid.closest), **ref, **param_arrays(cfg))
    print(f"sim {name} {mode}: seed {seed}, closest midpoint 2^{np.log2(mid.closest):.1f} over {mid.count} powers, gap {gap:.3g}, "
          f"resistance gap {rgap:.3g}, w in [{ref['w_final'].min():.4f}, {ref['w_final'].max():.4f}], "
          f"{distinct} distinct, {clipped:.2%} clipped, snapshots {ref['n_snapshots']}")


def main():
    for i, (name, cfg) in enumerate(R.SETS.items()):
        gen_update(name, cfg)
        for j, mode in enumerate(R.MODES):
            gen_sim(name, cfg, mode, 1000 * (4 * i + j + 1))


if __name__ == "__main__":
    main()
