"""GPU: Monte-Carlo device trials of the event-driven accumulator in one run (``nsof_accum_trials_dev``,
``simulate_trials``).

Yardsticks: the single-array path -- ``Accumulator(param_maps=planes[t])``, ``step(snap_every)``, ``w()``, ``resistance()``,
``block_current(memsize, snapshot=s)``, pinned by tests/test_accum_maps_gpu.py -- which every trial must equal EXACTLY (both
sides are the same device arithmetic), and the NumPy restatement tests/accum_maps_ref.py under the midpoint condition that
tests/test_accum_trials_cpu.py asserts for these inputs: states bit for bit, resistances within 1 ulp.  The seeded sensor is
7x37 with 40 slices -- it crosses a 32-slice group and the quad tail; with theta = 3 the groups are 16 slices;
``snapshot_every`` = 7 cuts the groups at the snapshot slices, ``memsize`` = 3 drops the remainder row and column."""
import functools

import numpy as np
import pytest

import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_params_ref as R  # noqa: N812
import accum_trials_cases as T  # noqa: N812
from conftest import ulp_diff

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def case_kw(case):
    c = K.CASES[case]
    return dict(version=c["version"], polarity=c["polarity"], active_v=K.ACTIVE_V, silent_v=c["silent_v"], params=K.PARAMS, dt=K.DT,
                refractory_us=c["refractory_us"], theta_events=c["theta"])


def single_array(ctx, case, maps, snap_every=T.SNAP_EVERY, memsize=T.MEMSIZE, kw=None, dense=None):
    """The existing path with one trial's planes (``None``: the uniform device) -> (w [A][H][W], resistance [A][H][W], block
    currents [A][S][rows][cols]).  ``dense``: as for ``Accumulator`` (``None`` automatic)."""
    from nsof.accumulator import Accumulator, slice_index_array
    kw = dict(case_kw(case) if kw is None else kw)
    ev, (H, W) = K.stream_of(case)  # noqa: N806
    acc = Accumulator(H, W, kw.pop("version"), kw.pop("polarity"), kw.pop("active_v"), kw.pop("silent_v"), ctx=ctx, param_maps=maps,
                      dense=dense, **kw)
    try:
        acc.step(*ev, slice_index_array(ev[3], 1000), snap_every=snap_every)
        arrays = range(2 if acc.split else 1)
        return (np.stack([acc.w(i) for i in arrays]), np.stack([acc.resistance(i) for i in arrays]),
                np.stack([np.stack([acc.block_current(memsize, which=i, snapshot=s) for s in range(acc.snapshot_count())]) for i in arrays]))
    finally:
        acc.close()


@functools.lru_cache(maxsize=None)
def run_of(nsof_lib, ctx, case, seeds):
    """One trial run of a (case, seeds) and the single-array run of each of its trials: computed once, shared."""
    maps, per = T.trial_maps(case, seeds)
    ev, shape = K.stream_of(case)
    got = nsof_lib.simulate_trials(ev, maps, sensor_size=shape, snapshot_every=T.SNAP_EVERY, memsize=T.MEMSIZE, ctx=ctx, **case_kw(case))
    return got, [single_array(ctx, case, m) for m in per]


def assert_trials_equal(got, singles, what):
    """Every trial, array and snapshot of a trial run against the single-array runs, exactly."""
    n_arr = singles[0][0].shape[0]
    assert got["w"].shape == (n_arr, len(singles)) + singles[0][0].shape[1:], what
    assert got["block_current"].shape == (n_arr, len(singles)) + singles[0][2].shape[1:], what
    assert got["w"].dtype == got["resistance"].dtype == F and got["block_current"].dtype == np.float64
    for t, (w, res, cur) in enumerate(singles):
        for a in range(n_arr):
            assert same_bits(got["w"][a, t], w[a]), (what, "w", t, a, int((bits(got["w"][a, t]) != bits(w[a])).sum()))
            assert same_bits(got["resistance"][a, t], res[a]), (what, "resistance", t, a)
            assert np.array_equal(got["block_current"][a, t].view(np.int64), cur[a].view(np.int64)), (what, "block_current", t, a)


@pytest.mark.parametrize("case,seeds", T.RUNS, ids=T.RUN_IDS)
def test_every_trial_equals_the_single_array_path(nsof_lib, ctx, case, seeds):
    got, singles = run_of(nsof_lib, ctx, case, seeds)
    assert_trials_equal(got, singles, case)
    H, W = K.SMALL  # noqa: N806
    assert got["block_current"].shape[2:] == ((40 - 1) // T.SNAP_EVERY + 1, H // T.MEMSIZE, W // T.MEMSIZE) == (6, 2, 12)
    assert not np.array_equal(got["w"][0, 0], got["w"][0, 1])                    # the trials differ
    assert (got["w"][0] != np.stack([m["wini"] for m in T.trial_maps(case, seeds)[1]])).any()
    if case == "small_v2_split":   # array B is driven by the p == 0 events and is an array of its own
        assert got["w"].shape[0] == 2 and (K.stream_of(case)[0][2] == 0).any()
        assert not np.array_equal(got["w"][0], got["w"][1]) and not np.array_equal(got["block_current"][0], got["block_current"][1])


@pytest.mark.parametrize("case,seeds", T.RUNS, ids=T.RUN_IDS)
def test_every_trial_equals_the_restatement(nsof_lib, ctx, case, seeds):
    got, _ = run_of(nsof_lib, ctx, case, seeds)
    for t, seed in enumerate(seeds):
        want, model, _ = T.restatement(case, seed, t)
        for a, wk in enumerate(("w_final", "w_final_b")[: got["w"].shape[0]]):
            differ = int((bits(got["w"][a, t]) != bits(want[wk])).sum())
            print(f"{case} trial {t} {wk}: {differ} of {want[wk].size} states differ from the restatement")
            assert differ == 0
            ulps = ulp_diff(got["resistance"][a, t], M.resistance_exp(want[wk], model))
            print(f"{case} trial {t} resistance of {wk}: at most {int(ulps.max())} ulp from the restatement")
            assert (ulps <= 1).all()


def test_shared_and_per_trial_planes_mix(nsof_lib, ctx):
    """kon and koff per trial, every other plane one [H][W] shared by the trials; then wini alone per trial, where the drives
    are one set for all trials."""
    case, seeds = "small_v1", (1, 3, 7)
    maps, per = T.trial_maps(case, seeds)
    ev, shape = K.stream_of(case)
    for varying in (("kon", "koff"), ("wini",)):
        mixed = {k: (v if k in varying else v[0]) for k, v in maps.items()}
        assert {v.ndim for v in mixed.values()} == {2, 3}
        got = nsof_lib.simulate_trials(ev, mixed, sensor_size=shape, snapshot_every=T.SNAP_EVERY, memsize=T.MEMSIZE, ctx=ctx, **case_kw(case))
        singles = [single_array(ctx, case, {k: (per[t][k] if k in varying else per[0][k]) for k in maps}) for t in range(len(seeds))]
        assert_trials_equal(got, singles, varying)
        assert not np.array_equal(got["w"][0, 0], got["w"][0, 1])


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split", "small_v1_leak"])
def test_one_trial_is_the_existing_path(nsof_lib, ctx, case):
    maps, per = T.trial_maps(case, (1,))
    ev, shape = K.stream_of(case)
    want = [single_array(ctx, case, per[0])]
    for planes in (maps, per[0]):   # [1][H][W] planes, and [H][W] planes alone
        got = nsof_lib.simulate_trials(ev, planes, sensor_size=shape, snapshot_every=T.SNAP_EVERY, memsize=T.MEMSIZE, ctx=ctx, **case_kw(case))
        assert_trials_equal(got, want, case)


@pytest.mark.parametrize("mode", list(R.MODES))
def test_constant_planes_give_the_uniform_accumulators_bits(nsof_lib, ctx, mode):
    """All 13 keys mapped to constant planes of the scalars, two trials: each is the uniform accumulator, bit for bit."""
    version, polarity, leak = R.MODES[mode]
    kw = dict(version=version, polarity=polarity, active_v=K.ACTIVE_V, silent_v=K.SET["leak_v"] if leak else 0.0, params=K.PARAMS, dt=K.DT,
              refractory_us=K.SET["refractory_us"])
    ev, shape = K.small_stream()
    maps = {k: np.full((2,) + shape, K.PARAMS[k], F) for k in R.KEYS}
    got = nsof_lib.simulate_trials(ev, maps, sensor_size=shape, snapshot_every=T.SNAP_EVERY, memsize=T.MEMSIZE, ctx=ctx, **kw)
    uniform = single_array(ctx, "small_v1", None, kw=kw)
    assert_trials_equal(got, [uniform, uniform], mode)
    assert len(np.unique(uniform[0])) > 10


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
@pytest.mark.parametrize("device", ["fitted", "alpha"])
def test_no_plane_at_all_is_the_uniform_accumulator(nsof_lib, ctx, case, device):
    """``param_maps={}``: one trial whose every key is a scalar -- the scalar-only route through the shared set-up kernel --
    for the fitted device (``params=None``) and for ``K.PARAMS``, schemes 1 and 2: the uniform ``Accumulator``'s state,
    resistance and block currents, bit for bit."""
    kw = case_kw(case) if device == "alpha" else dict(case_kw(case), params=None, dt=None)
    ev, shape = K.stream_of(case)
    got = nsof_lib.simulate_trials(ev, {}, sensor_size=shape, snapshot_every=T.SNAP_EVERY, memsize=T.MEMSIZE, ctx=ctx, **kw)
    uniform = single_array(ctx, case, None, kw=kw)
    assert got["w"].shape[1] == 1 and got["block_current"].shape[2] == 6
    assert_trials_equal(got, [uniform], (case, device))
    assert len(np.unique(uniform[0])) > 10 and not same_bits(uniform[0], np.full_like(uniform[0], 0.5))


@pytest.mark.parametrize("every,n_snaps", [(1, 40), (32, 2), (33, 2), (41, 1)])
@pytest.mark.parametrize("case", ["small_v1", "small_v1_theta3", "small_v2_split"])
def test_group_cuts_at_the_edges(nsof_lib, ctx, case, every, n_snaps):
    """A snapshot after every slice, at the 32-slice word boundary, one past it, and beyond the 40-slice stream (the
    other tests cut at 7 only).  Every trial equals the single array run with the event-pixel update (``dense=False``:
    groups of one mask word, 32 slices, 16 with theta = 3) and with the every-pixel pass (``dense=True``: scheme 1 takes
    two words, 64 and 32 slices) -- the shared ``group_len`` at both widths against the trial run's one."""
    seeds = (1, 3, 7)
    maps, per = T.trial_maps(case, seeds)
    ev, shape = K.stream_of(case)
    got = nsof_lib.simulate_trials(ev, maps, sensor_size=shape, snapshot_every=every, memsize=T.MEMSIZE, ctx=ctx, **case_kw(case))
    assert got["block_current"].shape[2] == n_snaps == (40 - 1) // every + 1
    for dense in (False, True):
        assert_trials_equal(got, [single_array(ctx, case, m, snap_every=every, dense=dense) for m in per], (case, every, dense))


def test_golden_stream(nsof_lib, ctx):
    """48x64, 200 slices, the study's cadence: a snapshot every 33 slices, 16 x 16 blocks."""
    case = "golden_v1"
    ev, shape = K.stream_of(case)
    per = [K.maps_of(shape, s) for s in (1, 3)]
    maps = {k: np.stack([m[k] for m in per]) for k in per[0]}
    got = nsof_lib.simulate_trials(ev, maps, sensor_size=shape, snapshot_every=33, memsize=16, ctx=ctx, **case_kw(case))
    assert got["block_current"].shape == (1, 2, (200 - 1) // 33 + 1, 3, 4)
    assert_trials_equal(got, [single_array(ctx, case, m, snap_every=33, memsize=16) for m in per], case)


def test_results_stay_on_the_device_and_block_currents_are_optional(nsof_lib, ctx, torch_dev):
    import torch
    case, seeds = "small_v1", (1, 3, 7)
    ev, shape = K.stream_of(case)
    dev = nsof_lib.simulate_trials_dev(ev, T.trial_maps(case, seeds)[0], sensor_size=shape, ctx=ctx, **case_kw(case))
    assert set(dev) == {"w", "resistance"} and all(isinstance(v, torch.Tensor) and v.is_cuda for v in dev.values())
    got, _ = run_of(nsof_lib, ctx, case, seeds)
    assert same_bits(dev["w"].cpu().numpy(), got["w"]) and same_bits(dev["resistance"].cpu().numpy(), got["resistance"])


def test_the_library_refuses_what_python_lets_through(nsof_lib, ctx):
    """An event outside the sensor and a bad scalar are the library's checks alone (NSOF_EINVAL, nothing launched)."""
    ev, shape = K.small_stream()
    ron = np.full((2,) + shape, 1e5, F)
    x = ev[0].copy()
    x[5] = shape[1]
    with pytest.raises(nsof_lib.error, match="outside"):
        nsof_lib.simulate_trials((x,) + ev[1:], dict(Ron=ron), sensor_size=shape, ctx=ctx)
    with pytest.raises(nsof_lib.error, match="von"):
        nsof_lib.simulate_trials(ev, dict(Ron=ron), sensor_size=shape, params=dict(K.PARAMS, von=-0.1), ctx=ctx)
