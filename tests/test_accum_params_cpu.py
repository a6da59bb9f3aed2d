"""CPU: the yardsticks of the parameterised accumulator and the Python layer around it.

tests/accum_params_ref.py (the NumPy restatement: float32 in the reference's order, powers and exp in float64 rounded once)
  * with the default parameters equals the C oracle's correctly rounded mode bit for bit on the existing element-wise golden
    inputs, and the C oracle's run of the `v1` golden within W_ATOL;
  * reproduces every golden made by running the reference with non-default parameters
    (tests/golden/gen_accum_params_golden.py).  Measured gaps, reference vs restatement (stored in each npz as `gap` /
    `res_gap`): update_state 5.96e-8 (1 ulp below 1) for both sets; simulate 0 for v1 / v2_split / v2_magnitude of both sets,
    5.96e-8 (alpha) and 2.98e-8 (wide) for the leak runs; resistances at most 2.31e-7 relative.  The bounds asserted are the
    project's own for the reference's SIMD pow / exp (1.2e-7 per step, W_ATOL per run, R_RTOL), not these figures;
  * meets the conditions the GPU tests rely on: closest midpoint approach of every simulate golden above 2^-40, fewer than
    0.1 % of the element-wise points closer than that, states away from the clip, and a frame-driven case whose float64 and
    long double evaluations agree within 1e-10.
Then the Python layer without a device: the parameter struct, keyword forwarding (stub accumulator), the metadata file."""
import gzip
import json

import numpy as np
import pytest

import accum_params_ref as R
from conftest import golden_path

F = np.float32
W_ATOL = 5e-7       # tests/test_accum_gpu.py
R_RTOL = 2e-6
STEP_ATOL = 1.2e-7  # the project's one-step tolerance against the reference's float32 pow
NEAR = 2.0 ** -40
SIM = [(s, m) for s in R.SETS for m in R.MODES]


def stored_params(d):
    return dict(zip([str(k) for k in d["param_keys"]], [float(v) for v in d["param_values"]]))


def run_restatement(d, mid=None):
    H, W = d["w_final"].shape  # noqa: N806
    return R.simulate(d["x"], d["y"], d["p"], d["t"], H, W, int(d["version"]), str(d["polarity"]), int(d["slice_us"]),
                      float(d["active_v"]), float(d["silent_v"]), stored_params(d), float(d["dt"]), int(d["refractory_us"]),
                      mid=mid)


def test_restatement_defaults_equal_correctly_rounded_oracle(oracle):
    g = np.load(golden_path("accum_update_state.npz"))
    for wk, vk in (("w_grid", "V_grid"), ("w_rand", "V_rand")):
        want, band = oracle.accum_update_state(g[wk], g[vk], rounding="correct")
        got = R.update_state(g[wk], g[vk])
        assert not band.any(), "an existing golden input lies in the device band"
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), wk
    want, band = oracle.accum_resistance(g["w_rand"], rounding="correct")
    got = R.resistance_exp(g["w_rand"])
    assert np.array_equal(got[~band], want[~band]) and band.sum() <= 1


def test_restatement_defaults_run_v1_golden_like_the_oracle(oracle):
    d = np.load(golden_path("accum_sim_v1.npz"))
    H, W = d["w_final"].shape  # noqa: N806
    ref = oracle.accum_simulate(d["x"], d["y"], d["p"], d["t"], H, W, 1, "split", 1000, -6.0, 0.0)
    got = R.simulate(d["x"], d["y"], d["p"], d["t"], H, W, 1, "split", 1000, -6.0, 0.0)
    assert got["resistances"].shape == ref["resistances"].shape
    assert np.abs(got["w_final"] - ref["w_final"]).max() <= W_ATOL
    assert (np.abs(got["resistances"] - ref["resistances"]) / ref["resistances"]).max() <= R_RTOL


def test_sets_are_what_the_issue_asks_for():
    a, w = R.SETS["alpha"], R.SETS["wide"]
    assert a["params"]["alphaoff"] != 1 and a["params"]["alphaon"] != 1 and float(a["params"]["boff"]).is_integer()
    d = R.DEFAULT
    assert w["params"]["voff"] < d["voff"] and w["params"]["von"] > d["von"]
    assert all(w["params"][k] != d[k] for k in ("Ron", "Roff", "wini"))
    assert all(s["dt"] != R.DT and s["refractory_us"] != R.REFRACTORY_US for s in (a, w))
    for s in (a, w):   # the leak voltage lies outside the set's dead zone
        assert s["leak_v"] < s["params"]["voff"] or s["leak_v"] > s["params"]["von"]


@pytest.mark.parametrize("name", list(R.SETS))
def test_restatement_reproduces_update_state_golden(name):
    d = np.load(golden_path(f"accum_params_update_{name}.npz"))
    p, dt = stored_params(d), float(d["dt"])
    assert p == {k: float(v) for k, v in R.SETS[name]["params"].items()} and dt == R.SETS[name]["dt"]
    got_g, dist_g = R.update_state(d["w_grid"], d["V_grid"], p, dt, return_distance=True)
    got_r, dist_r = R.update_state(d["w_rand"], d["V_rand"], p, dt, return_distance=True)
    assert np.array_equal(np.isnan(got_g), np.isnan(d["out_grid"])) and np.isnan(got_g).any()   # negative bases: nan alike
    gap = max(float(np.nanmax(np.abs(got_g - d["out_grid"]))), float(np.abs(got_r - d["out_rand"]).max()))
    print(f"{name}: update_state gap {gap:.3g} (stored {float(d['gap']):.3g})")
    assert gap <= float(d["gap"]) and gap <= STEP_ATOL
    # the grid covers what it is there for: the clip, and both neighbours of both thresholds
    assert (d["out_grid"] == 0).any() and (d["out_grid"] == 1).any()
    m = R.f32_model(p)
    for th in (m["voff"], m["von"]):
        assert {np.nextafter(th, F(-np.inf)), th, np.nextafter(th, F(np.inf))} <= set(d["V_grid"].ravel().tolist())
    # near-midpoint powers: the GPU test allows 1 ulp there; fewer than 0.1 % of the points
    near = int((dist_g < NEAR).sum() + (dist_r < NEAR).sum())
    assert near < 1e-3 * (dist_g.size + dist_r.size)
    for wk, rk in (("w_rand", "res_rand"), ("w_res", "res_grid")):
        rel = np.abs(R.resistance_exp(d[wk], p) - d[rk]) / d[rk]
        assert np.nanmax(rel) <= R_RTOL and np.nanmax(rel) <= float(d["res_gap"])


@pytest.mark.parametrize("name,mode", SIM)
def test_restatement_reproduces_simulate_golden(name, mode):
    d = np.load(golden_path(f"accum_params_sim_{name}_{mode}.npz"))
    cfg = R.SETS[name]
    assert stored_params(d) == {k: float(v) for k, v in cfg["params"].items()}
    assert float(d["dt"]) == cfg["dt"] and int(d["refractory_us"]) == cfg["refractory_us"]
    assert d["x"].size == 6000 and d["w_final"].shape == (48, 64)
    mid = R.Midpoints()
    got = run_restatement(d, mid)
    # the conditions on the case: no power closer than 2^-40 to a rounding midpoint, states away from the clip
    assert mid.closest > NEAR
    finals = np.concatenate([d[k].ravel() for k in ("w_final", "w_final_b") if k in d])
    assert ((finals == 0) | (finals == 1)).mean() < 0.01 and len(np.unique(finals)) >= 100
    if mode == "v1_leak":
        m = R.f32_model(cfg["params"])
        assert d["silent_v"] < m["voff"] or d["silent_v"] > m["von"]
    assert got["resistances"].shape[0] == int(d["n_snapshots"])
    idx = list(d["snap_idx"])
    gap = rgap = 0.0
    for k, rk in (("w_final", "resistances"), ("w_final_b", "resistances_b")):
        assert (k in d) == (k in got)
        if k in d:
            gap = max(gap, float(np.abs(got[k] - d[k]).max()))
            rgap = max(rgap, float((np.abs(got[rk][idx] - d[rk]) / d[rk]).max()))
    print(f"{name} {mode}: w gap {gap:.3g} (stored {float(d['gap']):.3g}), resistance gap {rgap:.3g}")
    assert gap <= float(d["gap"]) and gap <= W_ATOL and rgap <= R_RTOL


def test_frame_driven_case_is_insensitive():
    """The GPU test compares at 1e-9 (1000 sub-steps) and 1e-12 (10): the float64 restatement and its long double twin must
    agree far better than that, so the tolerance measures the device and not the case."""
    rng = np.random.default_rng(3)
    p = R.SETS["alpha"]["params"]
    for shape in ((4, 4), (9, 31)):
        imgs = rng.random((5,) + shape)
        for n_sub, tol in ((1000, 1e-10), (10, 1e-13)):
            w, res = R.simulate_frames(imgs, n_sub=n_sub, p=p)
            wl, resl = R.simulate_frames(imgs, n_sub=n_sub, p=p, dtype=np.longdouble)
            assert np.abs(w - wl.astype(np.float64)).max() <= tol
            assert (np.abs(res - resl.astype(np.float64)) / res).max() <= tol
            assert ((w > 0) & (w < 1)).mean() > 0.9 and np.ptp(w) > 0.05
    # default parameters: the oracle's frame loop
    from oracle import oracle as O  # noqa: N812
    O.build()
    imgs = rng.random((5, 4, 4))
    w, res = R.simulate_frames(imgs, n_sub=1000)
    wo, ro = O.accum_frames(imgs, n_sub=1000)
    assert np.abs(w - wo).max() <= 1e-12 and (np.abs(res - ro) / ro).max() <= 1e-12


# ---- the Python layer, without a device ----------------------------------------------------------------------------------
def test_params_struct_and_missing_key(nsof_lib):
    from nsof import accumulator as A
    from nsof.errors import NsofValueError
    ap = A.accum_params()
    assert [getattr(ap, k) for k in A._PARAM_KEYS] == [float(A.PARAMS[k]) for k in A._PARAM_KEYS]
    assert ap.dt == 5e-4 and ap.refractory_us == 800
    lib_default = nsof_lib._lib.AccumParams()
    nsof_lib._lib.load().nsof_accum_default_params(lib_default)
    assert bytes(lib_default) == bytes(ap)
    cfg = R.SETS["wide"]
    ap = A.accum_params(dict(cfg["params"], note="extra keys are ignored"), cfg["dt"], cfg["refractory_us"])
    assert ap.von == 0.25 and ap.wini == 0.35 and ap.dt == 2.5e-4 and ap.refractory_us == 45
    for key in A._PARAM_KEYS:
        p = {k: v for k, v in A.PARAMS.items() if k != key}
        with pytest.raises(NsofValueError, match=repr(key)):
            A.accum_params(p)
        with pytest.raises(NsofValueError, match=repr(key)):
            A.simulate((np.int16([1]), np.int16([1]), np.int8([1]), np.int64([0])), params=p)
    with pytest.raises(NsofValueError, match="voff"):
        A.accum_params(dict(A.PARAMS, voff="low"))
    with pytest.raises(NsofValueError):
        A.accum_params(refractory_us=0.5)
    with pytest.raises(NsofValueError):
        A.accum_params(params=[1, 2, 3])
    import inspect
    assert list(inspect.signature(A.update_state).parameters)[:4] == ["w", "V", "p", "dt"]
    assert list(inspect.signature(A.resistance_exp).parameters)[:2] == ["w", "p"]
    assert nsof_lib.PARAMS is A.PARAMS and nsof_lib.DT == 5e-4 and nsof_lib.REFRACTORY_US == 800
    assert A.PARAMS == R.DEFAULT


class _Stop(Exception):
    pass


def _stub(seen):
    class Stub:
        def __init__(self, *a, **kw):
            seen.append(kw)
            raise _Stop
    return Stub


def test_pipeline_forwards_the_model_keywords(nsof_lib, monkeypatch):
    import torch

    from nsof import accumulator, dist, gating, pipeline
    seen = []
    monkeypatch.setattr(pipeline, "Accumulator", _stub(seen))
    monkeypatch.setattr(accumulator, "Accumulator", _stub(seen))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    rng = np.random.default_rng(0)
    n = 400
    x, y = rng.integers(0, 32, n).astype(np.int16), rng.integers(0, 32, n).astype(np.int16)
    p, t = rng.integers(0, 2, n).astype(np.int8), np.sort(rng.integers(0, 100_000, n)).astype(np.int64)
    cfg = gating.dataset_config("uav") if hasattr(gating, "dataset_config") else None

    class Ctx:
        device = 0
    model = dict(params=dict(R.SETS["wide"]["params"]), dt=2.5e-4, refractory_us=45)
    calls = [lambda: pipeline.events_to_rois(x, y, p, t, (32, 32), cfg, ctx=Ctx(), **model),
             lambda: pipeline.events_to_rois_host(x, y, p, t, (32, 32), cfg, ctx=Ctx(), **model),
             lambda: pipeline.events_to_roi_flows(x, y, p, t, (32, 32), cfg, snapshot_every=10, ctx=Ctx(), **model)]
    # `params` of the flow-sequence pipelines is the Farneback parameter set: the device model goes in as accum_params
    seq = dict(accum_params=model["params"], dt=model["dt"], refractory_us=model["refractory_us"])
    calls.append(lambda: pipeline.events_to_flow_sequence(x, y, p, t, (32, 32), snapshot_every=10, ctx=Ctx(), **seq))
    monkeypatch.setattr(dist, "events_to_flow_sharded",
                        lambda x, y, p, t, hw, slice_us, every, band_frames, flow_of_frames, **k:
                        band_frames(x, y, p, t, np.arange(3), hw, every, 2))
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: False)
    calls.append(lambda: pipeline.events_to_flow_sequence_sharded(x, y, p, t, (32, 32), snapshot_every=10, ctx=Ctx(), **seq))
    band = dist.accumulator_band(2, "split", -6.0, 0.0, ctx=Ctx(), **model)
    calls.append(lambda: band(x, y, p, t, np.arange(3), (32, 32), (np.zeros(2, np.int64), np.zeros(2, np.int64))))
    for i, call in enumerate(calls):
        with pytest.raises(_Stop):
            call()
        assert len(seen) == i + 1, i
        kw = seen[-1]
        assert kw["params"] is model["params"] and kw["dt"] == 2.5e-4 and kw["refractory_us"] == 45, i
    # and nothing is invented when the caller passes nothing
    with pytest.raises(_Stop):
        pipeline.events_to_rois_host(x, y, p, t, (32, 32), cfg, ctx=Ctx())
    assert all(seen[-1][k] is None for k in ("params", "dt", "refractory_us"))


def test_metadata_records_what_was_used(nsof_lib, monkeypatch, tmp_path):
    from nsof import accumulator as A
    cfg = R.SETS["alpha"]

    class Stub:
        def __init__(self, H, W, version, polarity, active_v, silent_v, *, ctx=None, dense=None, params=None, dt=None,  # noqa: N803
                     refractory_us=None):
            ap = A.accum_params(params, dt, refractory_us)
            self.params, self.dt, self.refractory_us = A._params_dict(ap)
            self.split = version == 2 and polarity == "split"
            self.shape = (H, W)

        def step(self, *a, **k):
            pass

        def snapshots(self):
            return [np.ones((1,) + self.shape, F)] * (2 if self.split else 1)

        def w(self, which=0):
            return np.zeros(self.shape, F)

        def close(self):
            pass
    monkeypatch.setattr(A, "Accumulator", Stub)
    ev = (np.int16([1, 3]), np.int16([1, 2]), np.int8([1, 0]), np.int64([0, 1500]))
    A.simulate(ev, version=2, sensor_size=(4, 4), out_prefix=tmp_path / "run.x", params=cfg["params"], dt=cfg["dt"],
               refractory_us=cfg["refractory_us"])
    with gzip.open(tmp_path / "run.V2.json.gz", "rt") as fp:
        meta = json.load(fp)
    assert meta["dt"] == cfg["dt"] and meta["refractory_us"] == cfg["refractory_us"] and meta["theta_events"] is None
    assert meta["params"] == {k: float(v) for k, v in cfg["params"].items()}       # won / woff included
    assert set(meta["params"]) == set(A.PARAMS)
    A.simulate(ev, version=1, sensor_size=(4, 4), out_prefix=tmp_path / "dflt.x")
    with gzip.open(tmp_path / "dflt.V1.json.gz", "rt") as fp:
        meta = json.load(fp)
    assert meta["params"] == {k: float(v) for k, v in A.PARAMS.items()} and meta["dt"] == A.DT
    assert meta["refractory_us"] is None and meta["theta_events"] == 1
