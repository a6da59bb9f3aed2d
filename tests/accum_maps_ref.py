"""NumPy restatement of the synaptic accumulator with PER-PIXEL device parameters: ``accum_params_ref`` with array-valued
fields.  Nothing in the reference has parameter maps, so the yardstick is the project's own contract applied per pixel: every
field float32 (a mapped key's plane, or the scalar rounded once), dw/dt = (k * (V/v0 - 1) ** alpha) * (1 - w*s) ** b in that
order in float32, every power and exp evaluated in float64 from the float32 operands and rounded once, alpha == 1 taking no
power; neg_lam = float32(-ln(Roff / Ron)) with the logarithm in double of the values as held (a float32 plane widened, or
the scalar's double).  Feeds the same ``Midpoints`` collector as ``accum_params_ref``.
"""
import numpy as np

import accum_params_ref as R
from accum_params_ref import DT, F, KEYS, REFRACTORY_US, Midpoints, slice_bounds  # noqa: F401


def f32_model_maps(p=None, maps=None, dt=None):
    """The float32 device with ``maps`` (key -> [H][W]) in place of the scalars of ``p``: every key of ``KEYS`` as np.float32
    (a scalar) or a float32 plane, ``dt`` a scalar, ``neg_lam`` a plane as soon as Ron or Roff is one."""
    p = R.DEFAULT if p is None else p
    maps = {} if maps is None else maps
    assert all(k in KEYS for k in maps), "only the device parameters can be maps"
    m = {k: (np.array(maps[k], F) if k in maps else F(p[k])) for k in KEYS}
    m["dt"] = F(DT if dt is None else dt)
    ron, roff = (m[k].astype(np.float64) if k in maps else float(p[k]) for k in ("Ron", "Roff"))
    m["neg_lam"] = np.asarray(-np.log(roff / ron)).astype(F)[()]
    return m


def _is_model(p):
    return isinstance(p, dict) and "neg_lam" in p


def _planes(m, shape, keys):
    return [np.broadcast_to(np.asarray(m[k], F), shape) for k in keys]


def pow32(x32, b32):
    """x ** b for float32 operands, element by element: float64 power, rounded once (``accum_params_ref.pow32`` with an
    exponent per element)."""
    with np.errstate(all="ignore"):
        return np.power(np.asarray(x32, F).astype(np.float64), np.asarray(b32, F).astype(np.float64)).astype(F)


def _see(mid, x32, b32):
    if mid is not None and x32.size:
        mid.see(x32, b32 if b32.size > 1 else b32.reshape(-1)[0])


def _branch(w, V, v0, k, alpha, s, b, mid):  # noqa: N803
    """(k * (V/v0 - 1) ** alpha) * (1 - w*s) ** b on 1-D float32 arrays, all of one length."""
    a = V / v0 - F(1)
    pw = alpha != F(1)
    if pw.any():
        _see(mid, a[pw], alpha[pw])
        a = np.where(pw, pow32(a, alpha), a)
    base = F(1) - w * s
    _see(mid, base, b)
    return (k * a) * pow32(base, b)


def update_state(w, V, m, mid=None):  # noqa: N803
    """One step for float32 arrays [H][W]; ``m`` from ``f32_model_maps``.  ``mid``: a ``Midpoints`` to feed (with the powers
    of the pixels that evaluate them, as ``accum_params_ref.update_state`` feeds it)."""
    w = np.asarray(w, F)
    V = np.broadcast_to(np.asarray(V, F), w.shape)  # noqa: N806
    voff, von = _planes(m, w.shape, ("voff", "von"))
    off, on = V < voff, V > von
    dwdt = np.zeros(w.shape, F)
    with np.errstate(all="ignore"):
        for sel, names in ((off, ("voff", "koff", "alphaoff", "soff", "boff")), (on, ("von", "kon", "alphaon", "son", "bon"))):
            if sel.any():
                v0, k, alpha, s, b = (q[sel] for q in _planes(m, w.shape, names))
                dwdt[sel] = _branch(w[sel], V[sel], v0, k, alpha, s, b, mid)
        wn = w + dwdt * m["dt"]
        return np.where(wn < F(0), F(0), np.where(wn > F(1), F(1), wn)).astype(F)


def resistance_exp(w, m):
    w = np.asarray(w, F)
    with np.errstate(all="ignore"):
        e = np.exp((m["neg_lam"] * (F(1) - w)).astype(np.float64)).astype(F)
        return (np.asarray(m["Ron"], F).astype(np.float64) / e.astype(np.float64)).astype(F)


def surface_u8(w, m, mode="state"):
    """The 8-bit surface frame of states w, as ``accum_params_ref.surface_u8`` with the pixel's own resistance."""
    w = np.asarray(w, F)
    if mode == "state":
        g = (w * F(255)).astype(np.float64)
    else:
        r = resistance_exp(w, m).astype(np.float64)
        g = -3366.0 / np.log10(1.0 / r) - 306.0
    return np.clip(g, 0.0, 255.0).astype(np.uint8)


def surface_f32(w, m, mode="state"):
    """The same value clipped to [0, 255] and rounded to float32 instead of truncated."""
    w = np.asarray(w, F)
    if mode == "state":
        g = (w * F(255)).astype(np.float64)
    else:
        g = -3366.0 / np.log10(1.0 / resistance_exp(w, m).astype(np.float64)) - 306.0
    return np.clip(g, 0.0, 255.0).astype(F)


def simulate(x, y, pol, t, H, W, version, polarity, slice_us, active_v, silent_v, p=None, dt=None,  # noqa: N803
             refractory_us=None, mid=None, n_slices=None, maps=None, theta=1, states_every=None):
    """The slice loop of ``accum_params_ref.simulate`` on an array of per-pixel devices: the state starts at the ``wini`` plane
    where there is one; scheme 1 pulses a pixel in a slice that holds at least ``theta`` of its events.  Snapshots after every
    slice whose index is a multiple of max(1, nslices // 100); ``states_every``: also ``states``, array 0's state after
    every that many slices."""
    m = p if _is_model(p) else f32_model_maps(p, maps, dt)
    refr = REFRACTORY_US if refractory_us is None else int(refractory_us)
    x, y, pol, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(pol), np.asarray(t, np.int64)
    idx = slice_bounds(t, slice_us)
    total = len(idx) - 1
    every = max(1, total // 100)
    split = version == 2 and polarity == "split"
    narr = 2 if split else 1
    w = [np.array(np.broadcast_to(np.asarray(m["wini"], F), (H, W))) for _ in range(narr)]
    next_ok = [np.zeros((H, W), np.int64) for _ in range(narr)]
    snaps = [[] for _ in range(narr)]
    states = []
    sil = F(silent_v)
    act = F(active_v) if version == 1 else sil + F(active_v)
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
            w[i] = update_state(w[i], V, m, mid=mid)
            if s % every == 0:
                snaps[i].append(resistance_exp(w[i], m))
        if states_every and (s + 1) % states_every == 0:
            states.append(w[0].copy())
    out = dict(w_final=w[0], resistances=np.array(snaps[0], F).reshape(-1, H, W))
    if split:
        out.update(w_final_b=w[1], resistances_b=np.array(snaps[1], F).reshape(-1, H, W))
    if states_every:
        out["states"] = states
    return out
