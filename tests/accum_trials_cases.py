"""Inputs of the trial-run tests, shared by tests/test_accum_trials_cpu.py and tests/test_accum_trials_gpu.py: which (case,
map seeds) run, trial t's planes, and the restatement's run of every (case, trial) -- computed once, shared, never modified.

The cases, streams and ``maps_of`` are those of tests/accum_maps_cases.py; trial ``t`` of a run takes ``maps_of(shape,
seeds[t])``, stacked to ``[T][H][W]``.  The mixed case (``silent_v`` = -0.3) is built so that ONE trial leaves the dead zone:
trial 0 carries the checkerboard ``mixed_voff`` plane (half its pixels leak), every other trial a constant voff of -0.35,
below ``silent_v`` at every pixel -- alone, those trials would take the touched-pixels form.
"""
import functools

import numpy as np

import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_params_ref as R  # noqa: N812

F = np.float32
SMALL_CASES = [c for c in K.CASES if c.startswith("small_")]
# all six small cases with T = 3, two of them with T = 5 (no multiple of the update kernel's trial chunk)
RUNS = [(c, (1, 3, 7)) for c in SMALL_CASES] + [("small_v1", (1, 2, 3, 4, 5)), ("small_v2_split", (1, 2, 3, 4, 5))]
RUN_IDS = [f"{c}-T{len(s)}" for c, s in RUNS]
SNAP_EVERY, MEMSIZE = 7, 3


def trial_planes(case, seed, trial):
    """The planes of one trial, ``{key: float32 [H][W]}``."""
    _, shape = K.stream_of(case)
    maps = K.maps_of(shape, seed)
    if K.CASES[case].get("mixed"):
        maps["voff"] = K.mixed_voff(shape) if trial == 0 else np.full(shape, F(-0.35))
    return maps


@functools.lru_cache(maxsize=None)
def trial_maps(case, seeds):
    """-> (``{key: float32 [T][H][W]}``, the per-trial dicts it was stacked from)."""
    per = [trial_planes(case, s, i) for i, s in enumerate(seeds)]
    return {k: np.stack([m[k] for m in per]) for k in per[0]}, per


@functools.lru_cache(maxsize=None)
def restatement(case, seed, trial):
    """The NumPy restatement's run of one trial -> (its outputs, its float32 model, the closest midpoint approach)."""
    c = K.CASES[case]
    ev, (H, W) = K.stream_of(case)  # noqa: N806
    mid = R.Midpoints()
    model = M.f32_model_maps(K.PARAMS, trial_planes(case, seed, trial), K.DT)
    out = M.simulate(*ev, H, W, c["version"], c["polarity"], 1000, K.ACTIVE_V, c["silent_v"], model, refractory_us=c["refractory_us"],
                     mid=mid, theta=c["theta"])
    return out, model, mid.closest
