"""CPU: the host side of the event-driven trial run (``nsof_accum_trials_dev``, ``simulate_trials*``,
``pipeline.events_variability_dev``) -- the new symbols, the refusals that come before any device work, and the condition
on the inputs of tests/test_accum_trials_gpu.py under which the device must give the restatement's bits.  No GPU is
touched."""
import os
import re

import numpy as np
import pytest

import accum_maps_cases as K  # noqa: N812
import accum_trials_cases as T  # noqa: N812

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EV = (np.int16([1, 2, 3]), np.int16([1, 2, 0]), np.int8([1, 0, 1]), np.int64([0, 1500, 2500]))   # 6 x 8 sensor, 3 slices


def test_new_symbols_are_declared_exported_and_bound(nsof_lib):
    from nsof import _lib, pipeline
    header = open(os.path.join(ROOT, "include", "nsof.h")).read()
    lib = _lib.load()
    name = "nsof_accum_trials_dev"
    assert re.search(rf"\b{name}\s*\(", header)
    assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for f in ("simulate_trials", "simulate_trials_dev", "events_variability_dev"):
        assert callable(getattr(nsof_lib, f)), f
    assert nsof_lib.events_variability_dev is pipeline.events_variability_dev


@pytest.fixture
def no_device(monkeypatch, nsof_lib):
    """Any attempt to make a context or to call the library fails the test."""
    from nsof import accumulator as A  # noqa: N812
    from nsof import context

    def refused(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(A, "default_context", refused)
    monkeypatch.setattr(context, "default_context", refused)
    monkeypatch.setattr(A._lib, "load", refused)
    return nsof_lib


def test_refusals_come_before_any_device_work(no_device):
    from nsof import _lib
    nsof = no_device
    ok2, ok3 = np.full((6, 8), 0.1, F), np.full((2, 6, 8), 0.1, F)

    def refused(maps, match, status=None, **kw):
        for fn in (nsof.simulate_trials_dev, nsof.simulate_trials):
            with pytest.raises(nsof.error, match=match) as e:
                fn(EV, maps, sensor_size=(6, 8), **kw)
            assert isinstance(e.value, ValueError) and (status is None or e.value.status == status)
    refused(dict(von=ok3, son=np.full((3, 6, 8), 0.1, F)), "2.*3|3.*2", _lib.NSOF_ESHAPE)           # planes with differing T
    refused(dict(von=np.full((2, 6, 7), 0.1, F)), r"\(2, 6, 7\)", _lib.NSOF_ESHAPE)                 # [T][H][W] of the wrong H, W
    refused(dict(von=np.full((2, 8, 6), 0.1, F)), r"\(2, 8, 6\)", _lib.NSOF_ESHAPE)
    refused(dict(von=ok2.ravel()), "von", _lib.NSOF_ESHAPE)
    for bad in (np.nan, np.inf, -np.inf):                                                            # a non-finite value
        b = ok3.copy()
        b[1, 2, 3] = bad
        refused(dict(kon=b), "kon.*trial 1, row 2, column 3")
    for key, val in (("voff", 0.05), ("von", -0.1), ("von", 0.0), ("son", 1.5), ("soff", -0.25), ("wini", 2.0), ("Ron", -1.0),
                     ("Roff", 0.0)):                                                                 # ... or one outside its domain
        b = np.full((2, 6, 8), {"voff": -0.2, "Ron": 1e5, "Roff": 1e6}.get(key, 0.1), F)
        b[1, 4, 5] = val
        refused({key: b}, f"{key}.*trial 1, row 4, column 5")
        refused({key: b[1]}, f"{key}.*trial 0, row 4, column 5")                                     # a shared [H][W] plane: trial 0
    refused(dict(won=ok3), "won")                                                                    # an unknown key
    refused(dict(dt=ok2), "dt")
    refused([("von", ok3)], "mapping")
    refused(dict(von=ok3), "theta_events", version=2, theta_events=3)                                # theta with scheme 2
    refused(dict(von=ok3), "memsize", memsize=7)                                                     # larger than the 6 x 8 sensor
    refused(dict(von=ok3), "memsize", memsize=0)
    refused(dict(von=ok3), "snapshot_every", snapshot_every=0, memsize=2)
    refused(dict(von=ok3), "v_ds", v_ds=0.0, memsize=2)
    refused(dict(von=ok3), "version", version=3)
    refused(dict(von=ok3), "polarity", polarity="both")
    # simulate and Accumulator keep refusing 3-D planes
    with pytest.raises(nsof.error):
        nsof.simulate(EV, sensor_size=(6, 8), param_maps=dict(von=ok3))
    with pytest.raises(nsof.error):
        nsof.Accumulator(6, 8, param_maps=dict(von=ok3))


def test_the_study_refuses_before_any_device_work(no_device):
    nsof = no_device
    cfg = nsof.GatingConfig(MEMSIZE=2, THRES=240)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(nsof.error, match="trials"):
            nsof.events_variability_dev(*EV, (6, 8), cfg, dict(koff=0.1), bad)
    with pytest.raises(nsof.error, match="won"):
        nsof.events_variability_dev(*EV, (6, 8), cfg, dict(won=0.1), 2)


def test_plane_helper_gives_float32_planes_in_key_order(nsof_lib):
    from nsof.accumulator import trial_param_maps_arg
    assert trial_param_maps_arg(None) == (1, []) and trial_param_maps_arg({}) == (1, [])
    trials, maps = trial_param_maps_arg(dict(Ron=np.full((3, 2, 4), 1e5), son=np.full((2, 4), 0.25, F)), (2, 4))
    assert trials == 3 and [k for k, _ in maps] == ["son", "Ron"]
    assert [a.shape for _, a in maps] == [(1, 2, 4), (3, 2, 4)] and all(a.dtype == F and a.flags.c_contiguous for _, a in maps)


@pytest.mark.parametrize("case,seeds", T.RUNS, ids=T.RUN_IDS)
def test_gpu_runs_stay_away_from_rounding_midpoints(case, seeds):
    """The condition under which every trial of the GPU file must give the restatement's bits: no power of any trial's run
    within 2^-40 of a float32 rounding midpoint.  Also: the trials differ, and the mixed case is what it is there for."""
    finals = []
    for trial, seed in enumerate(seeds):
        out, model, closest = T.restatement(case, seed, trial)
        print(f"{case} seed {seed}: closest midpoint approach {closest:.3g} (bound {K.NEAR:.3g})")
        assert closest >= K.NEAR, (case, seed)
        assert len(np.unique(out["w_final"])) > 50
        finals.append(out["w_final"])
    assert all(not np.array_equal(finals[0], f) for f in finals[1:])
    maps, per = T.trial_maps(case, seeds)
    assert all(v.shape == (len(seeds),) + K.SMALL and v.dtype == F for v in maps.values())
    c = K.CASES[case]
    sil = F(c["silent_v"])
    leaks = [bool((sil < m["voff"]).any() or (sil > m["von"]).any()) for m in per]
    if c.get("mixed"):
        assert leaks == [True] + [False] * (len(seeds) - 1)        # one trial alone forces the every-pixel form
        assert (sil < per[0]["voff"]).any() and not (sil < per[0]["voff"]).all()
    elif case == "small_v1_leak":
        assert all(leaks)
    else:
        assert not any(leaks)
    if case == "small_v2_split":
        assert (K.stream_of(case)[0][2] == 0).any()                # array B is driven
