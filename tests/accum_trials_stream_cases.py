"""Inputs of the resumable trial accumulator's tests, shared by tests/test_accum_trials_stream_cpu.py and
tests/test_accum_trials_stream_gpu.py: where the 40-slice streams of tests/accum_maps_cases.py are cut, the documented group
rule restated (so that the CPU file can assert that the cuts land where they are said to), the per-trial voltages and the
restatement's run of a trial at its own operating point -- computed once, shared, never modified.
"""
import functools

import numpy as np

import accum_c2c_ref as N  # noqa: N812
import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_params_ref as R  # noqa: N812
import accum_trials_cases as T  # noqa: N812

F = np.float32
N_SLICES = 40
CASES = ["small_v1", "small_v1_theta3", "small_v2_split", "small_v2_magnitude", "small_v1_leak", "small_v1_mixed"]
SEEDS = (1, 2, 3, 4, 5)          # trial t of a T-trial run takes the planes of map seed SEEDS[t]
TRIALS = (1, 3, 5)               # the update kernel handles 4 trials per thread: 5 crosses that
# Two-chunk runs cut after k slices.  With a snapshot after slices 0, 7, 14, ...: 1 right after the first snapshot slice, 7 and
# 8 right before and after a later one, 31 / 32 / 33 around the 32 slices a mask word holds, 39 leaves a last chunk of one
# slice; 20 (theta = 3: 16 slices per word) is no multiple of that case's word.
CUTS = (1, 7, 8, 31, 32, 33, 39)
THETA3_CUT = 20
THREE_CHUNKS = (13, 33)          # chunks of 13, 20 and 7 slices
EMPTY_TAIL = 5                   # slices without events appended to the stream: a chunk that holds none
QUIET = dict(sigma=0.0, seed=0)  # the noisy restatement without noise is the noiseless one, bit for bit
# The noise of the per-trial-voltage runs: accum_c2c_ref.NOISE's spreads with a seed chosen, like the map seeds, on the
# RESTATEMENT alone -- no power of any of those runs comes closer than 2^-40 (relative) to a float32 rounding midpoint
# (asserted in the CPU file; with NOISE's own seed trial 2 at -8 V comes within 5.4e-13).
VOLT_NOISE = dict(sigma_on=0.05, sigma_off=0.1, seed=4)
ACTIVE_V = (-6.0, -4.0, -8.0, -6.0, -1.5)
LEAK_SILENT_V = (0.0, 0.0, K.SET["leak_v"], 0.0, 0.0)


def cuts_of(case):
    return CUTS + ((THETA3_CUT,) if K.CASES[case]["theta"] != 1 else ())


def word_slices(theta):
    """Slices per 32-bit mask word: 32 one-bit marks, or 32 // bits saturating counters of bits = ceil(log2(theta + 1))."""
    if theta == 1:
        return 32
    bits = 1
    while (1 << bits) < theta + 1:
        bits += 1
    return 32 // bits


def groups(counter, n_slices, theta, every):
    """The documented group rule: from absolute slice ``counter`` on, groups of up to a mask word's slices that end right
    after the next snapshot slice (absolute indices 0, every, 2 * every, ...) -> [(first, one past last)], absolute."""
    out, s, end = [], counter, counter + n_slices
    while s < end:
        g = min(end - s, word_slices(theta))
        if every > 0:
            to_snap = 1 if s % every == 0 else every - s % every + 1
            g = min(g, to_snap)
        out.append((s, s + g))
        s += g
    return out


def snaps_between(counter, n_slices, every):
    """Brute force: the snapshot slices among the n_slices slices from ``counter`` on."""
    return sum(1 for s in range(counter, counter + max(n_slices, 0)) if every >= 1 and s % every == 0)


def suppressed_after(case, k):
    """Scheme 2: the (array, pixel) pairs with an event in slice k whose pulse the refractory rule suppresses because of a
    pulse in an EARLIER slice -- the restatement's next_ok walk (accum_c2c_ref.simulate) without the states."""
    c = K.CASES[case]
    (x, y, pol, t), (H, W) = K.stream_of(case)  # noqa: N806
    x, y, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(t, np.int64)
    idx = M.slice_bounds(t, 1000)
    split = c["version"] == 2 and c["polarity"] == "split"
    found = set()
    for i in range(2 if split else 1):
        next_ok = np.zeros((H, W), np.int64)
        for s in range(k + 1):
            lo, hi = int(idx[s]), int(idx[s + 1])
            if hi <= lo:
                continue
            xs, ys = x[lo:hi], y[lo:hi]
            if split:
                keep = pol[lo:hi] == (1 if i == 0 else 0)
                xs, ys = xs[keep], ys[keep]
            ok = next_ok[ys, xs] <= t[lo]
            if s == k:
                found |= {(i, int(b), int(a)) for a, b in zip(xs[~ok], ys[~ok])}
            next_ok[ys[ok], xs[ok]] = t[hi - 1] + c["refractory_us"]
    return found


@functools.lru_cache(maxsize=None)
def restatement(case, trial, active_v, silent_v, noise_items, n_slices=None):
    """Trial ``trial`` (planes of map seed SEEDS[trial]) at its own voltages over the first ``n_slices`` slices -> (the
    restatement's outputs, its float32 model, the closest midpoint approach of any power of the run)."""
    c = K.CASES[case]
    ev, (H, W) = K.stream_of(case)  # noqa: N806
    mid = R.Midpoints()
    model = M.f32_model_maps(K.PARAMS, T.trial_planes(case, SEEDS[trial], trial), K.DT)
    out = N.simulate(*ev, H, W, c["version"], c["polarity"], 1000, active_v, silent_v, model, dict(noise_items), trial,
                     refractory_us=c["refractory_us"], mid=mid, theta=c["theta"], n_slices=n_slices)
    return out, model, mid.closest


def items(noise):
    return tuple(sorted(noise.items()))
