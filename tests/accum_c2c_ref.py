"""NumPy restatement of the trial run's cycle-to-cycle write noise, shared by tests/test_accum_c2c_cpu.py and
tests/test_accum_c2c_gpu.py: Philox4x32-10 and the variate in integer arithmetic, the noisy ``update_state`` and the slice
loop built on ``accum_maps_ref`` (``_branch``, ``f32_model_maps``, ``Midpoints``), per array and trial -- and which (case, map
seeds, spreads, noise seed) the GPU file runs, with the restatement of each computed once, shared, never modified.

The definition (include/nsof.h): xi is a pure function of (seed, array a, trial t, pixel = y * W + x, slice); the counter is
(pixel, slice & 0xffffffff, slice >> 32, t + 65536 * a), the key (seed & 0xffffffff, seed >> 32); S = the sum of the 16
output bytes, xi = float32(S - 2040) * float32(1 / sqrt(87380)); an update is w + (g * f) * dt with f = max(0, 1 + sigma *
xi), sigma that of the branch the drive took.
"""
import functools

import numpy as np

import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_params_ref as R  # noqa: N812
import accum_trials_cases as T  # noqa: N812

F = np.float32
U = np.uint64
MASK = U(0xFFFFFFFF)
M0, M1, W0, W1 = U(0xD2511F53), U(0xCD9E8D57), U(0x9E3779B9), U(0xBB67AE85)
C = F(float.fromhex("0x1.bb688cp-9"))

# What the GPU file runs against this restatement: all six small cases with T = 3, two of them with T = 5, per-trial planes
# and sigma_on = 0.05, sigma_off = 0.1; and once more with a spread of 0.5, where the clamp at 0 is reached.
# The noise seeds are chosen, like the map seeds, so that no power of a run comes closer than 2^-40 (relative) to a float32
# rounding midpoint (asserted in the CPU file): about every second seed qualifies for all 28 (case, trial) runs.
RUNS, RUN_IDS = T.RUNS, T.RUN_IDS
NOISE = dict(sigma_on=0.05, sigma_off=0.1, seed=0xC2C0000000000003)
CLAMP_RUN = ("small_v1_leak", (1, 3, 7))
CLAMP_NOISE = dict(sigma=0.5, seed=2024)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds on uint64 arrays that hold 32-bit words -> the four output words (uint64 arrays below 2**32)."""
    c0, c1, c2, c3 = (np.asarray(v, U) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = U(k0) & MASK, U(k1) & MASK
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> U(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> U(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def byte_sum(seed, array, trial, pixel, slice_):
    """S of the definition, int64, broadcast over ``pixel`` and ``slice_`` (Python ints or integer arrays, slice < 2**63)."""
    seed = int(seed)
    sl = np.asarray(slice_, U)
    words = philox4x32_10(np.asarray(pixel, U), sl & MASK, sl >> U(32), U(int(trial) + 65536 * int(array)), seed & 0xFFFFFFFF, seed >> 32)
    return sum(((w >> U(8 * j)) & U(0xFF)).astype(np.int64) for w in words for j in range(4))


def xi(seed, array, trial, pixel, slice_):
    """The variate, float32: one exact int -> float conversion, one rounded multiply."""
    return (byte_sum(seed, array, trial, pixel, slice_) - 2040).astype(F) * C


def spreads(noise):
    """(sigma_on, sigma_off, seed) of a ``c2c`` mapping as the tests write them."""
    if "sigma" in noise:
        return F(noise["sigma"]), F(noise["sigma"]), int(noise.get("seed", 0))
    return F(noise.get("sigma_on", 0.0)), F(noise.get("sigma_off", 0.0)), int(noise.get("seed", 0))


def update_state(w, V, m, sigma_on, sigma_off, x, mid=None, seen=None):  # noqa: N803
    """``accum_maps_ref.update_state`` with the step of every driven pixel scaled by f = max(0, 1 + sigma * xi): ``x`` the
    variates [H][W] of this (array, trial, slice).  ``seen``: a dict whose ``clamped`` becomes True when an evaluated update
    had 1 + sigma * xi < 0."""
    w = np.asarray(w, F)
    V = np.broadcast_to(np.asarray(V, F), w.shape)  # noqa: N806
    voff, von = M._planes(m, w.shape, ("voff", "von"))
    off, on = V < voff, V > von
    dwdt = np.zeros(w.shape, F)
    with np.errstate(all="ignore"):
        for sel, sigma, names in ((off, F(sigma_off), ("voff", "koff", "alphaoff", "soff", "boff")),
                                  (on, F(sigma_on), ("von", "kon", "alphaon", "son", "bon"))):
            if sel.any():
                v0, k, alpha, s, b = (q[sel] for q in M._planes(m, w.shape, names))
                g = M._branch(w[sel], V[sel], v0, k, alpha, s, b, mid)
                u = F(1) + sigma * x[sel]                       # the product rounded, then the sum
                if seen is not None and sigma != 0 and (u < 0).any():
                    seen["clamped"] = True
                dwdt[sel] = g * np.where(u < F(0), F(0), u)
        wn = w + dwdt * m["dt"]
        return np.where(wn < F(0), F(0), np.where(wn > F(1), F(1), wn)).astype(F)


def simulate(x, y, pol, t, H, W, version, polarity, slice_us, active_v, silent_v, m, noise, trial, refractory_us=None,  # noqa: N803
             mid=None, theta=1, n_slices=None):
    """The slice loop of ``accum_maps_ref.simulate`` for trial ``trial`` with the noise ``noise`` (a ``c2c`` mapping) ->
    ``dict(w_final[, w_final_b], clamped)``."""
    sigma_on, sigma_off, seed = spreads(noise)
    refr = M.REFRACTORY_US if refractory_us is None else int(refractory_us)
    x, y, pol, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(pol), np.asarray(t, np.int64)
    idx = M.slice_bounds(t, slice_us)
    total = len(idx) - 1
    split = version == 2 and polarity == "split"
    narr = 2 if split else 1
    w = [np.array(np.broadcast_to(np.asarray(m["wini"], F), (H, W))) for _ in range(narr)]
    next_ok = [np.zeros((H, W), np.int64) for _ in range(narr)]
    pixel = np.arange(H * W).reshape(H, W)
    sil = F(silent_v)
    act = F(active_v) if version == 1 else sil + F(active_v)
    seen = dict(clamped=False)
    for s in range(total if n_slices is None else n_slices):
        lo, hi = int(idx[s]), int(idx[s + 1])
        for i in range(narr):
            V = np.full((H, W), sil, F)  # noqa: N806
            if hi > lo:
                xs, ys = x[lo:hi], y[lo:hi]
                if split:
                    keep = pol[lo:hi] == (1 if i == 0 else 0)
                    xs, ys = xs[keep], ys[keep]
                if xs.size:
                    if version == 1:
                        counts = np.zeros((H, W), np.int64)
                        np.add.at(counts, (ys, xs), 1)
                        V[counts >= theta] = act
                    else:
                        ok = next_ok[i][ys, xs] <= t[lo]
                        V[ys[ok], xs[ok]] = act
                        next_ok[i][ys[ok], xs[ok]] = t[hi - 1] + refr
            w[i] = update_state(w[i], V, m, sigma_on, sigma_off, xi(seed, i, trial, pixel, s), mid=mid, seen=seen)
    out = dict(w_final=w[0], clamped=seen["clamped"])
    if split:
        out["w_final_b"] = w[1]
    return out


@functools.lru_cache(maxsize=None)
def _restatement(case, seed, trial, noise_items):
    c = K.CASES[case]
    ev, (H, W) = K.stream_of(case)  # noqa: N806
    mid = R.Midpoints()
    model = M.f32_model_maps(K.PARAMS, T.trial_planes(case, seed, trial), K.DT)
    out = simulate(*ev, H, W, c["version"], c["polarity"], 1000, K.ACTIVE_V, c["silent_v"], model, dict(noise_items), trial,
                   refractory_us=c["refractory_us"], mid=mid, theta=c["theta"])
    return out, model, mid.closest


def restatement(case, seed, trial, noise):
    """The noisy restatement's run of trial ``trial`` (planes of map seed ``seed``) -> (its outputs, its float32 model, the
    closest midpoint approach of any power of the run)."""
    return _restatement(case, seed, trial, tuple(sorted(noise.items())))
