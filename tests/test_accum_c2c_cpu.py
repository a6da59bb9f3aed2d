"""CPU: the host side of the trial run's cycle-to-cycle write noise (``nsof_accum_trials_c2c_dev``, ``nsof_accum_c2c_noise``,
``simulate_trials*(c2c=, trials=)``, ``c2c_noise``, ``events_variability_dev(c2c=)``) -- the generator against its known
answers, the library's host variate against the NumPy restatement bit for bit, its moments, the new symbols, the refusals
that come before any device work, and the conditions on the inputs of tests/test_accum_c2c_gpu.py under which the device
must give the restatement's bits.  No GPU is touched."""
import os
import re

import numpy as np
import pytest

import accum_c2c_ref as N  # noqa: N812
import accum_maps_cases as K  # noqa: N812

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EV = (np.int16([1, 2, 3]), np.int16([1, 2, 0]), np.int8([1, 0, 1]), np.int64([0, 1500, 2500]))   # 6 x 8 sensor, 3 slices


def words(ws):
    return " ".join(f"{int(w):08x}" for w in ws)


def test_philox_known_answers():
    f = 0xFFFFFFFF
    assert words(N.philox4x32_10(0, 0, 0, 0, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words(N.philox4x32_10(f, f, f, f, f, f)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(N.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0)) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_the_worked_example(nsof_lib):
    seed = 0x0123456789ABCDEF
    assert int(N.byte_sum(seed, 1, 2, 5, 7)) == 2180
    want = F(float.fromhex("0x1.e4fa5ap-2"))
    assert N.xi(seed, 1, 2, 5, 7) == want and N.xi(seed, 1, 2, 5, 7).dtype == F
    got = nsof_lib.c2c_noise(seed, 1, 2, 5, 7, 1)
    assert got.dtype == F and got.shape == (1,) and got[0] == want
    assert N.C.view(np.uint32) == 0x3B5DB446 and N.C == F(1.0 / np.sqrt(87380.0))


@pytest.mark.parametrize("seed", [0, 0x0123456789ABCDEF, 2**64 - 1])
def test_the_library_variate_is_the_restatement_bit_for_bit(nsof_lib, seed):
    """Pixel 2**32 - 1, a slice range that crosses 2**32, trial 65534 and array 1 included."""
    for array in (0, 1):
        for trial in (0, 2, 65534):
            for pixel in (0, 5, 258, 2**32 - 1):
                for first, n in ((0, 40), (2**32 - 4, 8), (2**40 + 3, 3)):
                    got = nsof_lib.c2c_noise(seed, array, trial, pixel, first, n)
                    want = N.xi(seed, array, trial, pixel, first + np.arange(n))
                    assert got.shape == want.shape == (n,)
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (array, trial, pixel, first)
    # the five arguments all matter
    base = nsof_lib.c2c_noise(seed, 0, 0, 0, 0, 64)
    for other in ((seed ^ 1, 0, 0, 0, 0), (seed ^ 2**32, 0, 0, 0, 0), (seed, 1, 0, 0, 0), (seed, 0, 1, 0, 0), (seed, 0, 0, 1, 0),
                  (seed, 0, 0, 0, 2**32)):
        assert not np.array_equal(base, nsof_lib.c2c_noise(*other, 64)), other
    assert nsof_lib.c2c_noise(seed, 0, 0, 0, 0, 0).shape == (0,)


def test_moments_of_65536_consecutive_draws(nsof_lib):
    x = nsof_lib.c2c_noise(99, 0, 0, 0, 0, 65536).astype(np.float64)
    print(f"mean {x.mean():.5f}, variance {x.var():.5f}, extremes {x.min():.3f} .. {x.max():.3f}")
    assert abs(x.mean()) < 0.02 and abs(x.var() - 1.0) < 0.02
    assert np.abs(x).max() <= 2040 * float(N.C) and len(np.unique(x)) > 1000


def test_new_symbols_are_declared_exported_and_bound(nsof_lib):
    from nsof import _lib, accumulator
    header = open(os.path.join(ROOT, "include", "nsof.h")).read()
    lib = _lib.load()
    for name in ("nsof_accum_trials_c2c_dev", "nsof_accum_c2c_noise"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert re.search(r"typedef struct nsof_accum_c2c\s*\{\s*uint64_t seed;\s*float sigma_on, sigma_off;\s*\} nsof_accum_c2c;", header)
    assert [f[0] for f in _lib.AccumC2c._fields_] == ["seed", "sigma_on", "sigma_off"]
    # the existing entry keeps its signature: the new one is that list plus the pointer
    assert _lib.SIGNATURES["nsof_accum_trials_c2c_dev"][1][:-1] == _lib.SIGNATURES["nsof_accum_trials_dev"][1]
    for f in ("c2c_noise", "c2c_arg"):
        assert getattr(nsof_lib, f) is getattr(accumulator, f)


def test_c2c_arg_forms(nsof_lib):
    c = nsof_lib.c2c_arg
    assert c(None) is None
    assert c(dict(sigma=0.05)) == (0, 0.05, 0.05)
    assert c(dict(sigma_on=0.25, seed=7)) == (7, 0.25, 0.0)
    assert c(dict(sigma_off=np.float32(0.5), sigma_on=0, seed=np.uint64(2**64 - 1))) == (2**64 - 1, 0.0, 0.5)
    assert c({}) == (0, 0.0, 0.0)


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


BAD_C2C = [
    (dict(sigma=0.1, gain=2), "gain"),                                  # unknown keys
    (dict(sigm=0.1), "sigm"),
    (dict(sigma=0.1, sigma_on=0.1), "both"),                            # sigma with a directional key
    (dict(sigma=0.1, sigma_off=0.0), "both"),
    (dict(sigma=-0.1), "sigma'.*-0.1"),                                 # negative, non-finite, no number
    (dict(sigma_on=-1e-9), "sigma_on"),
    (dict(sigma_off=float("nan")), "sigma_off"),
    (dict(sigma_on=float("inf")), "sigma_on"),
    (dict(sigma="0.1"), "sigma'.*not a number"),
    (dict(sigma_off=None), "sigma_off"),
    (dict(sigma=True), "sigma"),
    (dict(sigma=[0.1]), "sigma"),
    (dict(sigma=0.1, seed=-1), "seed"),                                 # a seed out of range
    (dict(sigma=0.1, seed=2**64), "seed"),
    (dict(sigma=0.1, seed=1.0), "seed"),
    (dict(sigma=0.1, seed="7"), "seed"),
    ([("sigma", 0.1)], "mapping"),
    (0.1, "mapping"),
]


def test_refusals_come_before_any_device_work(no_device):
    from nsof import _lib
    nsof = no_device
    ok3 = np.full((2, 6, 8), 0.1, F)
    for bad, match in BAD_C2C:
        for fn in (nsof.simulate_trials_dev, nsof.simulate_trials):
            with pytest.raises(nsof.error, match=match) as e:
                fn(EV, dict(von=ok3), sensor_size=(6, 8), c2c=bad)
            assert isinstance(e.value, ValueError), bad
        with pytest.raises(nsof.error, match=match):
            nsof.events_variability_dev(*EV, (6, 8), nsof.GatingConfig(MEMSIZE=2, THRES=240), dict(koff=0.1), 2, c2c=bad)
    for fn in (nsof.simulate_trials_dev, nsof.simulate_trials):
        for bad in (0, -3, 2.0, True, "4"):                              # trials
            with pytest.raises(nsof.error, match="trials"):
                fn(EV, None, sensor_size=(6, 8), trials=bad, c2c=dict(sigma=0.1))
        for t_planes in (2, 1):                                          # a [T'][H][W] plane with T' != T
            with pytest.raises(nsof.error, match=f"{t_planes} trials.*3") as e:
                fn(EV, dict(von=ok3[:t_planes]), sensor_size=(6, 8), trials=3)
            assert e.value.status == _lib.NSOF_ESHAPE
    for bad in ((-1, 0, 0, 0, 0, 1), (2**64, 0, 0, 0, 0, 1), (0, 2, 0, 0, 0, 1), (0, 0, 65535, 0, 0, 1), (0, 0, 0, 2**32, 0, 1),
                (0, 0, 0, 0, -1, 1), (0, 0, 0, 0, 0, -1)):
        with pytest.raises(nsof.error):
            nsof.c2c_noise(*bad)


RUNS = [(c, s, N.NOISE) for c, s in N.RUNS] + [N.CLAMP_RUN + (N.CLAMP_NOISE,)]
RUN_IDS = N.RUN_IDS + ["clamp"]


@pytest.mark.parametrize("case,seeds,noise", RUNS, ids=RUN_IDS)
def test_gpu_runs_stay_away_from_rounding_midpoints(case, seeds, noise):
    """The condition under which every trial of the GPU file must give the restatement's bits: no power of any trial's noisy
    run within 2^-40 of a float32 rounding midpoint.  The run with a spread of 0.5 really contains a clamped update (and none
    of the others does); the noise changes every trial's result."""
    import accum_trials_cases as T  # noqa: N812
    clamped = []
    for trial, seed in enumerate(seeds):
        out, _, closest = N.restatement(case, seed, trial, noise)
        print(f"{case} map seed {seed} trial {trial}: closest midpoint approach {closest:.3g} (bound {K.NEAR:.3g}), clamped {out['clamped']}")
        assert closest >= K.NEAR, (case, seed)
        clamped.append(out["clamped"])
        quiet = T.restatement(case, seed, trial)[0]
        assert not np.array_equal(out["w_final"], quiet["w_final"])
        assert len(np.unique(out["w_final"])) > 50
    assert any(clamped) == (noise is N.CLAMP_NOISE)


def test_the_noisy_restatement_without_noise_is_the_restatement():
    import accum_trials_cases as T  # noqa: N812
    for case in ("small_v1_leak", "small_v2_split"):
        out = N.restatement(case, 1, 0, dict(sigma=0.0, seed=5))[0]
        want = T.restatement(case, 1, 0)[0]
        for k in ("w_final", "w_final_b"):
            assert (k in want) == (k in out)
            if k in want:
                assert np.array_equal(out[k].view(np.uint32), want[k].view(np.uint32))
