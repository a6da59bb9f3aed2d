"""CPU: the resumable trial accumulator (``nsof_accum_trials``, ``nsof.TrialAccumulator``) as far as it goes without a device
-- Python's refusals come before a context exists, the new symbols are exported with the documented argument counts, the
snapshot count of a chunk against a brute-force count, and the properties claimed for the cuts and the voltages that
tests/test_accum_trials_stream_gpu.py runs (tests/accum_trials_stream_cases.py)."""
import os
import re

import numpy as np
import pytest

import accum_c2c_ref as N  # noqa: N812
import accum_maps_cases as K  # noqa: N812
import accum_trials_cases as T  # noqa: N812
import accum_trials_stream_cases as S  # noqa: N812
from conftest import ROOT

F = np.float32
EV = (np.int16([1, 2, 3]), np.int16([1, 2, 3]), np.int8([1, 0, 1]), np.int64([0, 1500, 2999]))

ARGS = {
    "nsof_accum_trials_create": 21, "nsof_accum_trials_destroy": 1, "nsof_accum_snaps_between": 3, "nsof_accum_trials_snaps_in": 2,
    "nsof_accum_trials_step": 9, "nsof_accum_trials_w_dev": 2, "nsof_accum_trials_resistance_dev": 2,
    "nsof_accum_trials_block_current_dev": 2, "nsof_accum_trials_surface_u8_dev": 6, "nsof_accum_trials_surface_f32_dev": 6,
    "nsof_accum_trials_read_state": 4, "nsof_accum_trials_write_state": 6, "nsof_accum_trials_reset": 1,
}


def test_new_symbols_are_declared_exported_and_bound(nsof_lib):
    from nsof import _lib, accumulator
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nsof.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, n_args in ARGS.items():
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert "typedef struct nsof_accum_trials nsof_accum_trials;" in header
    assert lib.nsof_abi_version() == 3                                   # new entries only
    assert nsof_lib.TrialAccumulator is accumulator.TrialAccumulator


@pytest.mark.parametrize("every", [1, 2, 7, 33])
def test_snapshot_count_of_a_chunk(nsof_lib, every):
    from nsof import _lib
    f = _lib.load().nsof_accum_snaps_between
    for counter in sorted({0, 1, every - 1, every, every + 1, 2 * every - 1, 2 * every, 2 * every + 1, 5 * every + 3, 2**40 * every - 1}):
        for n in sorted({0, 1, 2, every - 1, every, every + 1, 3 * every - 1, 3 * every, 3 * every + 1}):
            # (no brute force 2^40 cadences out: the count depends on the counter's residue alone)
            want = S.snaps_between(counter if counter < 2**20 else counter % every + every, n, every)
            assert f(counter, n, every) == want, (counter, n, every)
    # the whole run from 0 is the one-shot entry's S = (n - 1) // every + 1, and chunks add up to it
    for n in (1, 6, 7, 8, 40):
        assert f(0, n, every) == (n - 1) // every + 1
        for k in range(n + 1):
            assert f(0, k, every) + f(k, n - k, every) == f(0, n, every)
    assert f(0, 10, 0) == 0 and f(-1, 10, 7) == 0 and f(3, -2, 7) == 0    # no cadence, nonsense: no snapshot


def test_the_cuts_fall_where_they_are_said_to():
    """Against the documented group rule: the one-shot run's groups, and for each (case, k) whether the cut lies strictly
    inside one of them or right after a snapshot slice."""
    for case in S.CASES:
        theta = K.CASES[case]["theta"]
        whole = S.groups(0, S.N_SLICES, theta, T.SNAP_EVERY)
        assert whole[0] == (0, 1) and whole[-1][1] == S.N_SLICES and all(a[1] == b[0] for a, b in zip(whole, whole[1:]))
        assert all(1 <= e - s <= S.word_slices(theta) for s, e in whole)
        # every group but the last ends right after a snapshot slice or fills a word
        assert all((e - 1) % T.SNAP_EVERY == 0 or e - s == S.word_slices(theta) for s, e in whole[:-1])
        inside = [k for k in S.cuts_of(case) if any(s < k < e for s, e in whole)]
        after_snap = [k for k in S.cuts_of(case) if (k - 1) % T.SNAP_EVERY == 0]
        print(f"{case}: groups {whole}; cuts inside a group {inside}, right after a snapshot slice {after_snap}")
        assert inside and after_snap
        assert {1, 8} <= set(after_snap) and {7, 31, 32, 33, 39} <= set(inside)
        for k in S.cuts_of(case):
            # the chunked run regroups: its groups are the one-shot groups cut at k, and snapshots fall on the same slices
            first, second = S.groups(0, k, theta, T.SNAP_EVERY), S.groups(k, S.N_SLICES - k, theta, T.SNAP_EVERY)
            assert first[-1][1] == k == second[0][0] and second[-1][1] == S.N_SLICES
            ends = {e for _, e in first + second}
            assert {s + 1 for s in range(0, S.N_SLICES, T.SNAP_EVERY)} <= ends
            assert S.snaps_between(0, k, T.SNAP_EVERY) + S.snaps_between(k, S.N_SLICES - k, T.SNAP_EVERY) == 6
    assert S.word_slices(3) == 16 and S.THETA3_CUT % S.word_slices(3) != 0 and S.THETA3_CUT in S.cuts_of("small_v1_theta3")
    assert sum(np.diff((0,) + S.THREE_CHUNKS + (S.N_SLICES,)) == (13, 20, 7)) == 3


def test_the_refractory_rule_straddles_the_cut_at_8():
    """small_v2_split: 1200 us of refractory time against 1000 us slices -- in slice 8, the first after the cut, at least one
    pixel's pulse is suppressed by a pulse of an earlier slice, so next_ok has to survive the cut."""
    c = K.CASES["small_v2_split"]
    assert c["refractory_us"] == 1200 and c["version"] == 2
    found = S.suppressed_after("small_v2_split", 8)
    print(f"{len(found)} (array, row, column) suppressed in slice 8: {sorted(found)[:6]} ...")
    assert len(found) >= 1


def test_the_voltage_cases_are_what_they_claim():
    from nsof.accumulator import trial_voltage_arg
    assert len(S.ACTIVE_V) == len(S.LEAK_SILENT_V) == len(S.SEEDS) == 5
    _, per = T.trial_maps("small_v1", S.SEEDS)
    for t, m in enumerate(per):
        assert all((F(v) < m["voff"]).all() for v in S.ACTIVE_V)          # every active voltage writes (V < voff everywhere)
        zone = (F(S.LEAK_SILENT_V[t]) >= m["voff"]).all() and (F(S.LEAK_SILENT_V[t]) <= m["von"]).all()
        assert zone == (t != 2)                                           # trial 2 alone leaks
    assert trial_voltage_arg("active_v", S.ACTIVE_V, 5).dtype == F and trial_voltage_arg("active_v", -6, 5).shape == (1,)
    assert np.array_equal(trial_voltage_arg("v", np.float64([1, 2]), 2), F([1, 2]))


@pytest.mark.parametrize("case,noise", [("small_v1", S.QUIET), ("small_v1", S.VOLT_NOISE), ("small_v2_split", S.QUIET), ("small_v2_split", S.VOLT_NOISE)],
                         ids=["v1", "v1-noise", "v2", "v2-noise"])
def test_the_voltage_runs_stay_away_from_rounding_midpoints(case, noise):
    """The condition under which the GPU file demands the restatement's bits for the per-trial voltages (it applies the
    same rule itself: bit equality unless the closest approach is below the bound)."""
    for t, v in enumerate(S.ACTIVE_V):
        out, _, closest = S.restatement(case, t, v, 0.0, S.items(noise))
        print(f"{case} trial {t} at {v} V: closest midpoint approach {closest:.3g} (bound {K.NEAR:.3g}), clamped {out['clamped']}")
        assert closest >= K.NEAR, (case, t)
    ws = [S.restatement(case, t, v, 0.0, S.items(noise))[0]["w_final"] for t, v in enumerate(S.ACTIVE_V)]
    assert not np.array_equal(ws[0], S.restatement(case, 0, S.ACTIVE_V[1], 0.0, S.items(noise))[0]["w_final"])   # the voltage matters


def test_the_leaking_trial_stays_away_from_rounding_midpoints():
    for noise in (S.QUIET, S.VOLT_NOISE):
        for t, sv in enumerate(S.LEAK_SILENT_V):
            _, _, closest = S.restatement("small_v1", t, K.ACTIVE_V, sv, S.items(noise))
            print(f"small_v1 trial {t} silent {sv} V: closest midpoint approach {closest:.3g}")
            assert closest >= K.NEAR, t


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


BAD_VOLTS = [
    ([-6.0, -4.0], "2 voltages.*3 trials"), ([-6.0] * 4, "4 voltages.*3 trials"), ([], "0 voltages"), ([-6.0], "1 voltages"),
    ([-6.0, float("nan"), -4.0], r"\[1\].*finite"), (float("inf"), "finite"), ([-6.0, -4.0, 1e39], r"\[2\].*finite"),
    ("-6", "not a number"), (None, "not a number"), (True, "not a number"), ([-6.0, "x", -4.0], r"\[1\].*not a number"),
    (np.zeros((3, 1)), "neither a number nor a sequence"),
]


def test_python_refuses_before_a_context_exists(no_device):
    from nsof import _lib
    nsof = no_device
    ok3 = np.full((3, 6, 8), 0.1, F)
    for name in ("active_v", "silent_v"):
        for bad, match in BAD_VOLTS:
            with pytest.raises(nsof.error, match=match) as e:
                nsof.TrialAccumulator(6, 8, dict(von=ok3), **{name: bad})
            assert isinstance(e.value, ValueError), bad
            for fn in (nsof.simulate_trials_dev, nsof.simulate_trials):
                with pytest.raises(nsof.error, match=match):
                    fn(EV, dict(von=ok3), sensor_size=(6, 8), **{name: bad})
    with pytest.raises(nsof.error, match="2 voltages.*4 trials"):
        nsof.TrialAccumulator(6, 8, None, trials=4, active_v=[-6.0, -4.0])
    # ... and everything simulate_trials_dev refuses
    for kw, match in ((dict(version=3), "version"), (dict(polarity="both"), "polarity"), (dict(trials=0), "trials"),
                      (dict(c2c=dict(sigma=-1)), "sigma"), (dict(theta_events=0), "theta_events"), (dict(version=2, theta_events=3), "scheme 2"),
                      (dict(params=dict(voff=-0.2)), "lacks the key"), (dict(memsize=9, snapshot_every=7), "larger than"),
                      (dict(memsize=2), "needs snapshot_every"), (dict(memsize=0, snapshot_every=7), "memsize"),
                      (dict(memsize=2, snapshot_every=0), "snapshot_every"), (dict(memsize=2, snapshot_every=7, v_ds=0.0), "v_ds")):
        with pytest.raises(nsof.error, match=match):
            nsof.TrialAccumulator(6, 8, dict(von=ok3), **kw)
    with pytest.raises(nsof.error, match="von.*must be positive"):
        nsof.TrialAccumulator(6, 8, dict(von=-ok3))
    with pytest.raises(nsof.error, match="2 trials.*3") as e:
        nsof.TrialAccumulator(6, 8, dict(von=ok3[:2]), trials=3)
    assert e.value.status == _lib.NSOF_ESHAPE
    with pytest.raises(nsof.error, match=r"\(3, 5, 8\)") as e:
        nsof.TrialAccumulator(6, 8, dict(von=ok3[:, :5]))
    assert e.value.status == _lib.NSOF_ESHAPE
    # the study keeps one operating point
    for name in ("active_v", "silent_v"):
        with pytest.raises(nsof.error, match=f"{name}.*one number"):
            nsof.events_variability_dev(*EV, (6, 8), nsof.GatingConfig(MEMSIZE=2, THRES=240), dict(koff=0.1), 2, **{name: [-6.0, -4.0]})
