"""GPU: cycle-to-cycle write noise of the event-driven trial run (``nsof_accum_trials_c2c_dev``; ``simulate_trials*(c2c=,
trials=)``, ``events_variability_dev(c2c=)``).

Yardstick: the NumPy restatement tests/accum_c2c_ref.py under the midpoint condition that tests/test_accum_c2c_cpu.py
asserts for these inputs -- states bit for bit, resistances within 1 ulp -- on the six small cases of
tests/accum_maps_cases.py (7x37, 40 slices, 1500 events: a 32-slice group is crossed, theta = 3 makes 16-slice groups, T = 5
leaves a trial-chunk tail, ``memsize`` = 3 a remainder row and column; the leaking and the mixed case take the every-pixel
kernel, the others the touched-pixels one).  Everything else compares the device with itself: the variate is a pure
function of (seed, array, trial, pixel, slice), so nothing may depend on the grouping, the cadence or the trial count."""
import functools

import numpy as np
import pytest

import accum_c2c_ref as N  # noqa: N812
import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_trials_cases as T  # noqa: N812
from conftest import ulp_diff

pytestmark = pytest.mark.gpu

F = np.float32
OTHER = dict(sigma_on=0.05, sigma_off=0.1, seed=N.NOISE["seed"] + 1)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same(a, b):
    """Two result dicts, bit for bit (float32 states and resistances, float64 block currents)."""
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and
                                        np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def case_kw(case):
    c = K.CASES[case]
    return dict(version=c["version"], polarity=c["polarity"], active_v=K.ACTIVE_V, silent_v=c["silent_v"], params=K.PARAMS, dt=K.DT,
                refractory_us=c["refractory_us"], theta_events=c["theta"])


def run(nsof, ctx, case, maps, ev=None, snapshot_every=T.SNAP_EVERY, **kw):
    stream, shape = K.stream_of(case)
    return nsof.simulate_trials(stream if ev is None else ev, maps, sensor_size=shape, snapshot_every=snapshot_every, memsize=T.MEMSIZE,
                                ctx=ctx, **case_kw(case), **kw)


@functools.lru_cache(maxsize=None)
def _noisy(nsof, ctx, case, seeds, noise_items):
    return run(nsof, ctx, case, T.trial_maps(case, seeds)[0], c2c=dict(noise_items))


def noisy(nsof, ctx, case, seeds, noise):
    """One noisy trial run of a (case, map seeds, noise) with the per-trial planes: computed once, shared."""
    return _noisy(nsof, ctx, case, seeds, tuple(sorted(noise.items())))


@functools.lru_cache(maxsize=None)
def quiet(nsof, ctx, case, seeds):
    """The same run as the library gives it without the keyword."""
    return run(nsof, ctx, case, T.trial_maps(case, seeds)[0])


def assert_equals_the_restatement(got, case, seeds, noise):
    for t, seed in enumerate(seeds):
        want, model, _ = N.restatement(case, seed, t, noise)
        for a, wk in enumerate(("w_final", "w_final_b")[: got["w"].shape[0]]):
            differ = int((bits(got["w"][a, t]) != bits(want[wk])).sum())
            print(f"{case} trial {t} {wk}: {differ} of {want[wk].size} states differ from the restatement")
            assert differ == 0
            ulps = ulp_diff(got["resistance"][a, t], M.resistance_exp(want[wk], model))
            print(f"{case} trial {t} resistance of {wk}: at most {int(ulps.max())} ulp from the restatement")
            assert (ulps <= 1).all()


@pytest.mark.parametrize("case,seeds", N.RUNS, ids=N.RUN_IDS)
def test_every_trial_equals_the_restatement(nsof_lib, ctx, case, seeds):
    got = noisy(nsof_lib, ctx, case, seeds, N.NOISE)
    assert got["w"].shape == ((2 if case == "small_v2_split" else 1), len(seeds)) + K.SMALL
    assert_equals_the_restatement(got, case, seeds, N.NOISE)
    assert not np.array_equal(got["w"], quiet(nsof_lib, ctx, case, seeds)["w"])          # the noise is there


def test_the_clamped_run_equals_the_restatement(nsof_lib, ctx):
    case, seeds = N.CLAMP_RUN
    assert_equals_the_restatement(noisy(nsof_lib, ctx, case, seeds, N.CLAMP_NOISE), case, seeds, N.CLAMP_NOISE)


@pytest.mark.parametrize("case", ["small_v1", "small_v1_theta3", "small_v2_split", "small_v1_leak", "small_v1_mixed"])
def test_no_noise_is_the_noiseless_run(nsof_lib, ctx, case):
    seeds = (1, 3, 7)
    want = quiet(nsof_lib, ctx, case, seeds)
    assert set(want) == {"w", "resistance", "block_current"}
    maps = T.trial_maps(case, seeds)[0]
    for c2c in (None, dict(sigma=0.0), dict(sigma_on=0.0, sigma_off=0.0, seed=2**64 - 1), dict(seed=12345)):
        assert same(run(nsof_lib, ctx, case, maps, c2c=c2c), want), c2c


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
def test_a_spread_on_the_branch_no_drive_takes_changes_nothing(nsof_lib, ctx, case):
    """active_v = -6 takes the V < voff branch and silent_v = 0 lies in every dead zone: sigma_on meets no drive."""
    seeds = (1, 3, 7)
    maps, per = T.trial_maps(case, seeds)
    assert all((m["von"] > 0).all() and (K.ACTIVE_V < m["voff"]).all() for m in per)
    want = quiet(nsof_lib, ctx, case, seeds)
    assert same(run(nsof_lib, ctx, case, maps, c2c=dict(sigma_on=0.3, seed=9)), want)
    off = run(nsof_lib, ctx, case, maps, c2c=dict(sigma_off=0.3, seed=9))
    assert not np.array_equal(off["w"], want["w"]) and not np.array_equal(off["block_current"], want["block_current"])


@pytest.mark.parametrize("case", ["small_v1", "small_v1_theta3", "small_v2_split", "small_v1_mixed"])
def test_the_grouping_does_not_matter(nsof_lib, ctx, case):
    """A snapshot after every slice (groups of one), every 7 and every 40 slices (whole mask words): the same final states."""
    seeds = (1, 3, 7)
    maps = T.trial_maps(case, seeds)[0]
    want = noisy(nsof_lib, ctx, case, seeds, N.NOISE)
    for every in (1, 40):
        got = run(nsof_lib, ctx, case, maps, snapshot_every=every, c2c=N.NOISE)
        assert got["block_current"].shape[2] == (40 - 1) // every + 1
        assert np.array_equal(bits(got["w"]), bits(want["w"])) and np.array_equal(bits(got["resistance"]), bits(want["resistance"])), every


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
def test_snapshots_are_the_noisy_state_at_their_slice(nsof_lib, ctx, case):
    """The stream cut after snapshot slice s runs to the state the full run had there: that state in an ``Accumulator``
    with the trial's planes gives ``block_current[a][t][s / 7]`` of the full run."""
    from nsof.accumulator import Accumulator
    seeds = (1, 3, 7)
    maps, per = T.trial_maps(case, seeds)
    full = noisy(nsof_lib, ctx, case, seeds, N.NOISE)
    ev, (H, W) = K.stream_of(case)  # noqa: N806
    kw = case_kw(case)
    for snap in (2, 5):                                  # slices 14 (first mask word) and 35 (second)
        s = snap * T.SNAP_EVERY
        keep = ev[3] < (s + 1) * 1000
        assert ev[3][0] == 0 and (ev[3][keep] >= s * 1000).any()      # the cut stream's last slice is slice s
        cut = run(nsof_lib, ctx, case, maps, ev=tuple(a[keep] for a in ev), c2c=N.NOISE)
        assert cut["block_current"].shape[2] == snap + 1
        for t in range(len(seeds)):
            acc = Accumulator(H, W, kw["version"], kw["polarity"], kw["active_v"], kw["silent_v"], ctx=ctx, param_maps=per[t],
                              params=kw["params"], dt=kw["dt"], refractory_us=kw["refractory_us"], theta_events=kw["theta_events"])
            try:
                for a in range(full["w"].shape[0]):
                    acc.load_state(dict(w=cut["w"][a, t]), which=a)
                    got = acc.block_current(T.MEMSIZE, which=a)
                    assert np.array_equal(got.view(np.int64), full["block_current"][a, t, snap].view(np.int64)), (snap, t, a)
                    assert np.array_equal(got.view(np.int64), cut["block_current"][a, t, snap].view(np.int64))
            finally:
                acc.close()
    assert not np.array_equal(full["block_current"][:, :, 2], full["block_current"][:, :, 5])


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split", "small_v1_leak"])
def test_trials_of_identical_devices_differ_by_their_noise_alone(nsof_lib, ctx, case):
    """No plane at all, ``trials=T``: the trials differ pairwise, and trial t does not depend on how many trials run."""
    four = run(nsof_lib, ctx, case, None, trials=4, c2c=N.NOISE)
    assert four["w"].shape[1] == four["resistance"].shape[1] == four["block_current"].shape[1] == 4
    for a in range(four["w"].shape[0]):
        for i in range(4):
            for j in range(i):
                assert not np.array_equal(four["w"][a, i], four["w"][a, j]), (a, i, j)
    three, five = run(nsof_lib, ctx, case, {}, trials=3, c2c=N.NOISE), run(nsof_lib, ctx, case, None, trials=5, c2c=N.NOISE)
    for k in three:
        assert np.array_equal(three[k].view(np.uint8), five[k][:, :3].view(np.uint8)), k
        assert np.array_equal(four[k].view(np.uint8), five[k][:, :4].view(np.uint8)), k
    # without noise identical devices stay identical, and a shared [H][W] plane counts as no trial axis
    plain = run(nsof_lib, ctx, case, dict(wini=np.full(K.SMALL, 0.25, F)), trials=3)
    assert plain["w"].shape[1] == 3 and all(np.array_equal(bits(plain["w"][:, 0]), bits(plain["w"][:, t])) for t in (1, 2))


def test_the_seed_decides(nsof_lib, ctx):
    case, seeds = "small_v2_split", (1, 3, 7)
    maps = T.trial_maps(case, seeds)[0]
    first = noisy(nsof_lib, ctx, case, seeds, N.NOISE)
    assert same(run(nsof_lib, ctx, case, maps, c2c=dict(N.NOISE)), first)
    other = run(nsof_lib, ctx, case, maps, c2c=OTHER)
    high = run(nsof_lib, ctx, case, maps, c2c=dict(N.NOISE, seed=N.NOISE["seed"] ^ 2**63))      # the key's second word
    for o in (other, high):
        assert all(not np.array_equal(o["w"][a, t], first["w"][a, t]) for a in range(2) for t in range(3))
    assert not np.array_equal(other["w"], high["w"])


def test_the_library_refuses_a_bad_spread(nsof_lib, ctx):
    """What Python refuses first, asked of the library itself: NSOF_EINVAL naming the field and the value."""
    import ctypes as C

    from nsof import _lib
    from nsof.accumulator import accum_params, slice_index_array
    ev, (H, W) = K.small_stream()  # noqa: N806
    idx = slice_index_array(ev[3], 1000)
    w = np.zeros(1, F)   # never written: the call is refused before anything is allocated or launched
    for field, value, text in (("sigma_on", -0.5, "-0.5"), ("sigma_off", float("nan"), "nan"), ("sigma_off", float("inf"), "inf")):
        c2c = _lib.AccumC2c(1, 0.1, 0.1)
        setattr(c2c, field, value)
        rc = ctx._lib.nsof_accum_trials_c2c_dev(ctx.ptr, H, W, 1, 0, -6.0, 0.0, C.byref(accum_params()), 1, ev[0].ctypes.data,
                                                ev[1].ctypes.data, ev[2].ctypes.data, ev[3].ctypes.data, idx.ctypes.data, len(idx) - 1, 7, 0,
                                                1.0, 1, 0, None, None, None, w.ctypes.data, w.ctypes.data, None, C.byref(c2c))
        assert rc == _lib.NSOF_EINVAL
        msg = ctx._lib.nsof_last_error(ctx.ptr).decode()
        assert field in msg and text in msg, msg


def test_the_study_with_noise(nsof_lib, ctx):
    """``events_variability_dev(rel_sigma={}, c2c=)``: identical devices, the trial run all the same; the nominal array stays
    noiseless.  Without ``c2c`` an empty ``rel_sigma`` still reproduces the nominal run in every trial."""
    trials, case = 4, "small_v1"
    ev, (H, W) = K.stream_of(case)  # noqa: N806
    cfg = nsof_lib.GatingConfig(MEMSIZE=T.MEMSIZE, THRES=240)
    common = dict(slice_us=1000, snapshot_every=T.SNAP_EVERY, ctx=ctx, **case_kw(case))
    out = {k: v.cpu().numpy() for k, v in nsof_lib.events_variability_dev(*ev, (H, W), cfg, {}, trials, c2c=N.NOISE, **common).items()}
    rows, cols, n = H // T.MEMSIZE, W // T.MEMSIZE, 6
    want = run(nsof_lib, ctx, case, None, trials=trials, c2c=N.NOISE)["block_current"][0]
    assert out["stacks"].shape == (trials, n, rows, cols) and np.array_equal(out["stacks"].view(np.int64), want.view(np.int64))
    base = {k: v.cpu().numpy() for k, v in nsof_lib.events_variability_dev(*ev, (H, W), cfg, {}, trials, **common).items()}
    assert np.array_equal(out["nominal"].view(np.int64), base["nominal"].view(np.int64))
    assert out["nominal"].shape == (n, rows, cols) and out["nominal"].dtype == out["stacks"].dtype == np.float64
    assert out["counts"].shape == (n, rows, cols) and out["counts"].dtype == np.int32
    assert np.array_equal(out["p_gate"], out["counts"] / trials)
    assert out["flips"].shape == out["rect_counts"].shape == (trials, n) and out["rects"].shape == (trials, n, 32, 4)
    assert all(not np.array_equal(out["stacks"][t], out["nominal"]) for t in range(trials))
    # without the keyword: what it returned before -- every trial the nominal run
    assert base.keys() == out.keys()
    assert all(np.array_equal(base["stacks"][t].view(np.int64), base["nominal"].view(np.int64)) for t in range(trials))
    assert not base["flips"].any()
    # ... and with a spread, the trial run of the drawn planes
    from nsof.accumulator import variability_maps
    sigma = dict(koff=0.1, Ron=0.1)
    spread = nsof_lib.events_variability_dev(*ev, (H, W), cfg, sigma, trials, seed=3, **common)["stacks"].cpu().numpy()
    planes = variability_maps(H, W, sigma, K.PARAMS, 3, trials=trials)
    assert np.array_equal(spread.view(np.int64), run(nsof_lib, ctx, case, planes)["block_current"][0].view(np.int64))
