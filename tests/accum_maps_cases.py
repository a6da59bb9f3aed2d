"""Inputs of the parameter-map tests, shared by tests/test_accum_maps_cpu.py and tests/test_accum_maps_gpu.py: the event
streams, the maps, and the restatement's run of every case (computed once, shared, never modified).

Streams: the stored ones of tests/golden/accum_params_sim_alpha_*.npz (their own 48x64 sensor, 200 slices) and a seeded random
one on 7x37 -- 259 pixels, no multiple of 4: the quad tail and the quads that straddle rows -- of 40 slices of 1000 us with a
hot set of pixels that collects several events per (pixel, slice) cell, so that a count threshold matters, and event times
dense enough that many gaps are shorter than the refractory time.

The seeds are chosen so that no power of a case comes closer than 2^-40 (relative) to a float32 rounding midpoint in the
restatement's long double evaluation: a condition on the inputs (asserted in the CPU file), under which the device, whose
series are accurate to ~4e-14, must give the restatement's bits.
"""
import functools

import numpy as np

import accum_maps_ref as M  # noqa: N812
import accum_params_ref as R  # noqa: N812
from conftest import golden_path

F = np.float32
NEAR = 2.0 ** -40
SET = R.SETS["alpha"]
PARAMS, DT = SET["params"], SET["dt"]
SMALL = (7, 37)
# 10 % spread on the rate constants, the thresholds, the resistances, one s and one b, and on the initial state
SIGMA = {k: 0.1 for k in ("kon", "koff", "von", "voff", "Ron", "Roff", "son", "boff", "wini")}


def maps_of(shape, seed):
    from nsof.accumulator import variability_maps
    return variability_maps(shape[0], shape[1], SIGMA, PARAMS, seed)


@functools.lru_cache(maxsize=None)
def golden_stream(mode):
    d = np.load(golden_path(f"accum_params_sim_alpha_{mode}.npz"))
    return (d["x"], d["y"], d["p"], d["t"]), tuple(d["w_final"].shape)


@functools.lru_cache(maxsize=None)
def small_stream(seed=5, n_ev=1500, n_slices=40):
    rng = np.random.default_rng(seed)
    H, W = SMALL  # noqa: N806
    hot = rng.choice(H * W, 40, replace=False)
    pix = np.where(rng.random(n_ev) < 0.6, rng.choice(hot, n_ev), rng.integers(0, H * W, n_ev))
    t = np.sort(rng.integers(0, n_slices * 1000, n_ev)).astype(np.int64)
    t[0], t[-1] = 0, n_slices * 1000 - 1
    return ((pix % W).astype(np.int16), (pix // W).astype(np.int16), rng.integers(0, 2, n_ev).astype(np.int8), t), SMALL


def mixed_voff(shape):
    """A voff plane with values on both sides of silent_v = -0.3: a checkerboard of -0.25 (the pixel leaks) and -0.35 (idle
    pixels keep their bits)."""
    yy, xx = np.indices(shape)
    return np.where((yy + xx) % 2 == 0, F(-0.25), F(-0.35)).astype(F)


# name -> stream ("golden:<mode>" / "small"), scheme, polarity, silent_v, theta, refractory_us, seed of the maps
CASES = {
    "golden_v1": dict(stream="golden:v1", version=1, polarity="split", silent_v=0.0, theta=1, refractory_us=20, seed=1),
    "golden_v2_split": dict(stream="golden:v2_split", version=2, polarity="split", silent_v=0.0, theta=1, refractory_us=20, seed=1),
    "small_v1": dict(stream="small", version=1, polarity="split", silent_v=0.0, theta=1, refractory_us=20, seed=1),
    "small_v1_theta3": dict(stream="small", version=1, polarity="split", silent_v=0.0, theta=3, refractory_us=20, seed=1),
    "small_v2_split": dict(stream="small", version=2, polarity="split", silent_v=0.0, theta=1, refractory_us=1200, seed=1),
    "small_v2_magnitude": dict(stream="small", version=2, polarity="magnitude", silent_v=0.0, theta=1, refractory_us=1200, seed=1),
    "small_v1_leak": dict(stream="small", version=1, polarity="split", silent_v=SET["leak_v"], theta=1, refractory_us=20, seed=1),
    "small_v1_mixed": dict(stream="small", version=1, polarity="split", silent_v=-0.3, theta=1, refractory_us=20, seed=1, mixed=True),
}
ACTIVE_V = -6.0


def stream_of(case):
    s = CASES[case]["stream"]
    return small_stream() if s == "small" else golden_stream(s.split(":")[1])


@functools.lru_cache(maxsize=None)
def case_maps(case):
    c = CASES[case]
    _, shape = stream_of(case)
    maps = maps_of(shape, c["seed"])
    if c.get("mixed"):
        maps["voff"] = mixed_voff(shape)
    return maps


@functools.lru_cache(maxsize=None)
def restatement(case):
    """-> (the restatement's run with array 0's state after every slice in ``states``, its float32 model, the closest midpoint
    approach of any power of the run)."""
    c = CASES[case]
    ev, (H, W) = stream_of(case)  # noqa: N806
    mid = R.Midpoints()
    model = M.f32_model_maps(PARAMS, case_maps(case), DT)
    out = M.simulate(*ev, H, W, c["version"], c["polarity"], 1000, ACTIVE_V, c["silent_v"], model, refractory_us=c["refractory_us"],
                     mid=mid, theta=c["theta"], states_every=1)
    return out, model, mid.closest
