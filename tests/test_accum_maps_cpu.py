"""CPU: per-pixel parameter maps -- the restatement tests/accum_maps_ref.py against tests/accum_params_ref.py, the inputs of
tests/test_accum_maps_gpu.py, the host helper ``variability_maps`` and the Python-side rejections.  No GPU is touched."""
import numpy as np
import pytest

import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_params_ref as R  # noqa: N812
from conftest import golden_path

F = np.float32
SIM = [(s, m) for s in R.SETS for m in R.MODES]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def golden_run(name, mode):
    """(stream, shape, the keyword arguments both restatements take) of one stored simulate case."""
    d = np.load(golden_path(f"accum_params_sim_{name}_{mode}.npz"))
    H, W = d["w_final"].shape  # noqa: N806
    cfg = R.SETS[name]
    args = (d["x"], d["y"], d["p"], d["t"], H, W, int(d["version"]), str(d["polarity"]), 1000, float(d["active_v"]), float(d["silent_v"]))
    return args, (H, W), cfg


@pytest.mark.parametrize("name,mode", SIM)
def test_constant_planes_equal_the_uniform_restatement(name, mode):
    args, shape, cfg = golden_run(name, mode)
    want = R.simulate(*args, cfg["params"], cfg["dt"], cfg["refractory_us"])
    maps = {k: np.full(shape, cfg["params"][k], F) for k in R.KEYS}
    got = M.simulate(*args, cfg["params"], cfg["dt"], cfg["refractory_us"], maps=maps)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert len(np.unique(want["w_final"])) > 10
    for mode_s in ("state", "current"):
        assert np.array_equal(M.surface_u8(want["w_final"], M.f32_model_maps(cfg["params"], maps, cfg["dt"]), mode_s),
                              R.surface_u8(want["w_final"], cfg["params"], mode_s))


@pytest.mark.parametrize("mode", list(R.MODES))
def test_two_class_label_map_equals_the_per_class_runs(mode):
    """Left half of the array the set "alpha", right half the set "wide" (dt, refractory time and the voltages of "alpha"):
    every pixel equals the uniform run of its own class."""
    args, shape, cfg = golden_run("alpha", mode)
    left = np.zeros(shape, bool)
    left[:, : shape[1] // 2] = True
    pa, pw = R.SETS["alpha"]["params"], R.SETS["wide"]["params"]
    maps = {k: np.where(left, F(pa[k]), F(pw[k])).astype(F) for k in R.KEYS}
    got = M.simulate(*args, pa, cfg["dt"], cfg["refractory_us"], maps=maps)
    runs = [R.simulate(*args, p, cfg["dt"], cfg["refractory_us"]) for p in (pa, pw)]
    for k in got:
        want = np.where(left, runs[0][k], runs[1][k])
        assert np.array_equal(bits(got[k]), bits(want)), k
    assert not np.array_equal(runs[0]["w_final"], runs[1]["w_final"])


@pytest.mark.parametrize("case", list(K.CASES))
def test_gpu_cases_stay_away_from_rounding_midpoints(case):
    """The condition under which the device must give the restatement's bits: no power of the run within 2^-40 of a float32
    rounding midpoint.  Also: the case does what it is there for."""
    out, model, closest = K.restatement(case)
    c = K.CASES[case]
    (x, y, p, t), (H, W) = K.stream_of(case)  # noqa: N806
    print(f"{case}: closest midpoint approach {closest:.3g} (bound {K.NEAR:.3g})")
    assert closest >= K.NEAR
    assert len(out["states"]) == len(R.slice_bounds(t, 1000)) - 1
    assert len(np.unique(out["w_final"])) > 50 and (out["w_final"] != model["wini"]).any()
    if c["stream"] == "small":
        assert H * W % 4 and W % 4
        cells = np.unique((t // 1000 * H + y) * W + x, return_counts=True)[1]
        assert (cells >= 3).sum() >= 10 and (cells == 1).sum() >= 100   # a threshold of 3 keeps some cells and drops most
        assert (np.diff(t) < c["refractory_us"]).sum() >= 10
    if c["theta"] > 1:
        one = M.simulate(x, y, p, t, H, W, 1, "split", 1000, K.ACTIVE_V, c["silent_v"], model)
        assert not np.array_equal(one["w_final"], out["w_final"])
    if c.get("mixed"):
        voff = K.case_maps(case)["voff"]
        assert (voff > F(c["silent_v"])).any() and (voff < F(c["silent_v"])).any()


def test_variability_maps():
    from nsof.accumulator import PARAMS, _PARAM_KEYS, variability_maps
    sig = {k: 0.1 for k in ("Roff", "kon", "voff", "wini", "bon")}
    a = variability_maps(9, 13, sig, seed=3)
    b = variability_maps(9, 13, dict(reversed(list(sig.items()))), seed=3)
    assert set(a) == set(sig) and all(v.dtype == F and v.shape == (9, 13) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in sig)                       # deterministic, whatever the key order
    assert not np.array_equal(a["kon"], variability_maps(9, 13, sig, seed=4)["kon"])
    assert np.std(a["Roff"]) / PARAMS["Roff"] == pytest.approx(0.1, rel=0.3)
    # the draw of a key does not depend on which later keys are asked for
    assert np.array_equal(variability_maps(9, 13, {"alphaoff": 0.1, "wini": 0.2}, seed=3)["alphaoff"],
                          variability_maps(9, 13, {"alphaoff": 0.1}, seed=3)["alphaoff"])
    # a spread as large as the value itself stays inside the model's domain
    wide = variability_maps(40, 50, {k: 1.0 for k in _PARAM_KEYS}, R.SETS["wide"]["params"], seed=1)
    tiny = np.finfo(F).tiny
    assert all(np.isfinite(v).all() for v in wide.values())
    assert (wide["voff"] <= -tiny).all() and (wide["von"] >= tiny).all() and (wide["koff"] > 0).all() and (wide["kon"] < 0).all()
    assert all((wide[k] >= 0).all() and (wide[k] <= 1).all() for k in ("son", "soff", "wini"))
    assert (wide["Ron"] >= tiny).all() and (wide["Roff"] >= tiny).all()
    assert (wide["voff"] == -tiny).any() and (wide["son"] == 0).any() and (wide["soff"] == 1).any()   # the clip is reached
    # no spread: constant planes of the float32 value
    flat = variability_maps(5, 6, {k: 0.0 for k in _PARAM_KEYS}, R.SETS["alpha"]["params"])
    assert all(np.array_equal(flat[k], np.full((5, 6), F(R.SETS["alpha"]["params"][k]))) for k in _PARAM_KEYS)
    from nsof.errors import NsofValueError
    with pytest.raises(NsofValueError, match="won"):
        variability_maps(5, 6, {"won": 0.1})


def test_python_side_rejections_need_no_gpu(monkeypatch):
    """Unknown keys, a wrong shape and non-finite values are refused before a context is created or the library is called."""
    import nsof
    from nsof import accumulator as A  # noqa: N812
    from nsof.errors import NsofValueError

    def no_context(*a, **k):
        raise AssertionError("a context was asked for")
    monkeypatch.setattr(A, "default_context", no_context)
    monkeypatch.setattr(A._lib, "load", no_context)
    ok = np.full((6, 8), 0.1, F)
    ev = (np.int16([1, 2]), np.int16([1, 2]), np.int8([1, 0]), np.int64([0, 1500]))
    nan = ok.copy()
    nan[2, 3] = np.nan
    inf = ok.copy()
    inf[5, 7] = -np.inf
    bad = [({"won": ok}, "won"), ({"woff": ok}, "woff"), ({"dt": ok}, "dt"), ({"refractory_us": ok}, "refractory_us"),
           ({"Rof": ok}, "Rof"), ({"von": ok[:5]}, r"\(5, 8\)"), ({"von": ok.T}, r"\(8, 6\)"), ({"von": ok.ravel()}, "von"),
           ({"von": 0.1}, "von"), ({"kon": nan}, r"\[2\]\[3\]"), ({"Ron": inf}, r"\[5\]\[7\]"), ([("von", ok)], "mapping"),
           ({"von": [["a"] * 8] * 6}, "von")]
    for maps, match in bad:
        with pytest.raises(NsofValueError, match=match):
            A.Accumulator(6, 8, param_maps=maps)
        with pytest.raises(NsofValueError, match=match):
            nsof.simulate(ev, sensor_size=(6, 8), param_maps=maps)
    assert A.param_maps_arg(None) == [] and A.param_maps_arg({}) == []
    got = A.param_maps_arg({"wini": ok.astype(np.float64).tolist(), "alphaoff": ok}, (6, 8))
    assert [k for k, _ in got] == ["alphaoff", "wini"] and all(a.dtype == F and a.flags.c_contiguous for _, a in got)
