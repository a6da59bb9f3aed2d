"""NumPy float64 restatement of nsof_flow_ensemble_dev (include/nsof.h), and the shared case list
of its tests.  The trials are folded by a sequential loop, one NumPy operation per arithmetic step, so every addition
happens in the kernel's order and nothing is fused: sum, sq, epe2_max and the counts must match the device bit for bit.
aee is the correctly rounded pixel sum (math.fsum) over the pixel count: the device's fixed-order sum is held to it
within the worst case of any summation order (aee_bound)."""
import math
import os
import re

import numpy as np

from conftest import PKG

# (T, F, H, W) of the kernel tests; the last two are sized from the tile constants, see kernel_cases()
_FIXED_CASES = [(1, 1, 1, 1), (5, 2, 19, 37)]


def tile_constant(name):
    """An integer `constexpr int NAME = value;` of csrc/flow_ensemble.hip."""
    with open(os.path.join(PKG, "csrc", "flow_ensemble.hip")) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


def kernel_cases():
    """The fixed cases; one with three workgroups in x and in y whose last tiles hold one pixel / one row, and more trials
    than one batch of loads plus a tail; one with an even width (the 16-byte loads without the odd-width extra load), two
    workgroups in x and a lane tail."""
    bx, by, inflight = (tile_constant(k) for k in ("FE_BX", "FE_BY", "FE_INFLIGHT"))
    return _FIXED_CASES + [(inflight + 2, 2, 2 * by + 1, 2 * bx + 1), (3, 1, by + 1, bx + 2)]


def strides(case, padded):
    """(row, field, trial) strides in floats of the flows of a case: dense, or padded so that odd widths get rows that
    start 16-byte aligned (and even widths lose that alignment)."""
    t, f, h, w = case
    rs = 2 * w + (6 if padded else 0)
    fs = h * rs + (4 if padded else 0)
    return rs, fs, f * fs + (8 if padded else 0)


def load_form(case, padded):
    """The load form nsof_flow_ensemble_dev picks for a 16-byte aligned base: "px" (8-byte loads), "pair" (16-byte loads)
    or "pair_odd" (16-byte loads plus the last pixel of an odd row)."""
    t, f, h, w = case
    rs, fs, ts = strides(case, padded)
    pairs = w >= 2 and rs % 4 == 0 and (f == 1 or fs % 4 == 0) and (t == 1 or ts % 4 == 0)
    return "px" if not pairs else "pair_odd" if w % 2 else "pair"


def geometry(case):
    """(workgroups in x, in y, pixels of the last x tile, rows of the last y tile, lanes of a wave with a lone first pixel)."""
    t, f, h, w = case
    bx, by = tile_constant("FE_BX"), tile_constant("FE_BY")
    gx, gy = -(-w // bx), -(-h // by)
    return gx, gy, w - (gx - 1) * bx, h - (gy - 1) * by, w % tile_constant("FE_PX")


def make_flows(case, seed):
    """Seeded flows [T][F][H][W][2] and a reference [F][H][W][2], float32 in +-20 px."""
    rng = np.random.default_rng(seed)
    t, f, h, w = case
    return (rng.uniform(-20, 20, (t, f, h, w, 2)).astype(np.float32), rng.uniform(-20, 20, (f, h, w, 2)).astype(np.float32))


def fold(flows, ref=None, tau=1.0, state=None):
    """flows float32 [T][F][H][W][2], ref float32 [F][H][W][2] or None -> dict(sum, sq, epe2_max, aee, outliers, nonfinite,
    n_trials) as nsof.flow_ensemble_dev returns them; state: a previous result to continue (left unchanged)."""
    flows = np.asarray(flows)
    assert flows.dtype == np.float32 and flows.ndim == 5 and flows.shape[-1] == 2
    n_t, n_f, h, w = flows.shape[:4]
    r = np.zeros((n_f, h, w, 2)) if ref is None else np.asarray(ref).astype(np.float64)
    if state is None:
        s, q, m, done = np.zeros((n_f, h, w, 2)), np.zeros((n_f, h, w, 3)), np.zeros((n_f, h, w)), 0
    else:
        s, q, m, done = state["sum"].copy(), state["sq"].copy(), state["epe2_max"].copy(), state["n_trials"]
    aee = np.empty((n_t, n_f))
    outliers, nonfinite = np.empty((n_t, n_f), np.int32), np.empty((n_t, n_f), np.int32)
    tau2 = float(tau) * float(tau)
    with np.errstate(all="ignore"):
        for t in range(n_t):
            d = flows[t].astype(np.float64) - r
            du, dv = d[..., 0], d[..., 1]
            uu, vv = du * du, dv * dv
            s[..., 0] += du
            s[..., 1] += dv
            q[..., 0] += uu
            q[..., 1] += vv
            q[..., 2] += du * dv
            e2 = uu + vv
            m = np.where(e2 > m, e2, m)
            outliers[t] = (e2 > tau2).sum(axis=(1, 2))
            nonfinite[t] = (~(e2 < np.inf)).sum(axis=(1, 2))
            e = np.sqrt(e2)
            for f in range(n_f):
                # fsum has no answer for inf - inf; sqrt(e2) is never negative, and a NaN or inf makes the sum non-finite anyway
                aee[t, f] = (math.fsum(e[f].ravel()) if np.isfinite(e[f]).all() else e[f].sum()) / (w * h)
    return dict(sum=s, sq=q, epe2_max=m, aee=aee, outliers=outliers, nonfinite=nonfinite, n_trials=done + n_t)


def aee_bound(w, h):
    """Relative bound of the device's aee against fold()'s: a sum of W*H non-negative terms in ANY order is within
    (W*H - 1) * 2^-53 of the exact sum (each of the W*H - 1 additions rounds a partial sum that is at most the total), the
    square roots add one ulp, and the final division and fsum's own rounding one more each: (W*H + 2) * 2^-53."""
    return (w * h + 2) * 2.0 ** -53
