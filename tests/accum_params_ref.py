"""NumPy restatement of the synaptic accumulator with the device model as an argument: the yardstick of the
parameterised entries (oracle/accum_ref.c has the fitted constants built in).

float32 forms -- ``update_state``, ``resistance_exp``, ``simulate`` (scheme 1, scheme 2 split / magnitude), ``surface_u8``
-- follow the GPU's stated contract: every parameter rounded to float32 once, dw/dt = (k * (V/v0 - 1) ** alpha) *
(1 - w*s) ** b in that order in float32, every power and exp evaluated in float64 FROM THE FLOAT32 OPERANDS and rounded
once (alpha == 1 takes no power).  ``simulate_frames`` is the float64 frame-driven loop.

``Midpoints`` collects, from an ``np.longdouble`` evaluation of the same powers, the closest relative approach of any
power to a float32 rounding midpoint: where it is larger than the device's series error the device must give the same
bits as this file.
"""
import numpy as np

F = np.float32
KEYS = ("alphaoff", "alphaon", "voff", "von", "koff", "kon", "son", "soff", "bon", "boff", "Ron", "Roff", "wini")
DEFAULT = dict(alphaoff=1, alphaon=1, voff=-0.2, von=0.1, koff=51.03, kon=-2.91, son=0.2, soff=0.8, bon=-5.12, boff=3.10,
               Ron=163_305, Roff=2_104_377, won=1, woff=0, wini=0.5)
DT = 5e-4
REFRACTORY_US = 800

# The non-default devices of the tests (tests/golden/accum_params_*.npz were generated with them).
#   alpha: alphaoff, alphaon != 1, an integer boff, another dt and refractory time
#   wide : a wider dead zone [-0.6, 0.25], other Ron / Roff / wini, another dt and refractory time
SETS = {
    "alpha": dict(params=dict(alphaoff=1.5, alphaon=2, voff=-0.25, von=0.15, koff=0.25, kon=-0.05, son=0.3, soff=0.7,
                              bon=-4.5, boff=3, Ron=163_305, Roff=2_104_377, won=1, woff=0, wini=0.5),
                  dt=4e-4, refractory_us=20, active_v=-6.0, leak_v=0.4),
    "wide": dict(params=dict(alphaoff=1, alphaon=1, voff=-0.6, von=0.25, koff=4.0, kon=-3.3, son=0.25, soff=0.75,
                             bon=-4.7, boff=2.6, Ron=120_000.0, Roff=3_300_000.0, won=1, woff=0, wini=0.35),
                 dt=2.5e-4, refractory_us=45, active_v=-6.0, leak_v=-0.9),
}
# name -> (version, polarity, silent voltage: None = 0, "leak" = the set's leak_v)
MODES = {"v1": (1, "split", None), "v2_split": (2, "split", None), "v2_magnitude": (2, "magnitude", None),
         "v1_leak": (1, "split", "leak")}


def f32_model(p=None, dt=None):
    """The float32 device: every key of ``KEYS`` and ``dt`` as np.float32, neg_lam = float32(-ln(Roff / Ron)) with the
    logarithm taken in double of the unrounded values (np.log of two Python numbers)."""
    p = DEFAULT if p is None else p
    m = {k: F(p[k]) for k in KEYS}
    m["dt"] = F(DT if dt is None else dt)
    m["neg_lam"] = F(-np.log(float(p["Roff"]) / float(p["Ron"])))
    return m


class Midpoints:
    """Closest relative approach of a power to a float32 rounding midpoint, over everything passed to ``see``."""

    def __init__(self):
        self.closest = np.inf
        self.count = 0

    @staticmethod
    def distance(x32, b32):
        """Per element: |pow - nearest float32 midpoint| / |pow| from a long double power of the float32 operands
        (inf where the power is 0, subnormal as float32, infinite or nan: nothing is rounded there that could go two ways)."""
        L = np.longdouble
        with np.errstate(all="ignore"):
            pw = np.power(np.asarray(x32, F).astype(L), L(F(b32)))
            f = pw.astype(F)
            lo = np.nextafter(f, F(-np.inf)).astype(L)
            hi = np.nextafter(f, F(np.inf)).astype(L)
            fl = f.astype(L)
            d = np.minimum(np.abs(pw - (fl + lo) / 2), np.abs(pw - (fl + hi) / 2)) / np.abs(pw)
        ok = np.isfinite(pw) & np.isfinite(f) & (np.abs(f) >= np.finfo(F).tiny) & np.isfinite(d)
        return np.where(ok, d, np.inf).astype(np.float64)

    def see(self, x32, b32):
        d = self.distance(x32, b32)
        if d.size:
            self.closest = min(self.closest, float(d.min()))
            self.count += d.size
        return d


def pow32(x32, b32):
    """x ** b for float32 operands: float64 power, rounded once."""
    with np.errstate(all="ignore"):
        return np.power(np.asarray(x32, F).astype(np.float64), np.float64(F(b32))).astype(F)


def _branch(w, V, v0, k, alpha, s, b, mid, dist):
    a = V / v0 - F(1)
    if alpha != F(1):
        if mid is not None:
            d = mid.see(a, alpha)
            if dist is not None:
                dist[0] = np.minimum(dist[0], d)
        a = pow32(a, alpha)
    base = F(1) - w * s
    if mid is not None:
        d = mid.see(base, b)
        if dist is not None:
            dist[0] = np.minimum(dist[0], d)
    return (k * a) * pow32(base, b)


def update_state(w, V, p=None, dt=None, mid=None, return_distance=False):  # noqa: N803
    """One step for float32 arrays.  ``mid``: a ``Midpoints`` to feed.  ``return_distance``: also the per-element closest
    midpoint approach of the powers the element evaluated (inf where it evaluated none)."""
    m = p if isinstance(p, dict) and "neg_lam" in p else f32_model(p, dt)
    w = np.asarray(w, F)
    V = np.asarray(V, F)  # noqa: N806
    dwdt = np.zeros(w.shape, F)
    dist_all = np.full(w.shape, np.inf)
    if return_distance and mid is None:
        mid = Midpoints()
    with np.errstate(all="ignore"):
        for sel, v0, k, alpha, s, b in ((V < m["voff"], m["voff"], m["koff"], m["alphaoff"], m["soff"], m["boff"]),
                                        (V > m["von"], m["von"], m["kon"], m["alphaon"], m["son"], m["bon"])):
            if sel.any():
                dist = [np.full(int(sel.sum()), np.inf)]
                dwdt[sel] = _branch(w[sel], V[sel], v0, k, alpha, s, b, mid, dist if return_distance else None)
                dist_all[sel] = dist[0]
        wn = w + dwdt * m["dt"]
        out = np.where(wn < F(0), F(0), np.where(wn > F(1), F(1), wn)).astype(F)   # nan stays nan, as np.clip leaves it
    return (out, dist_all) if return_distance else out


def resistance_exp(w, p=None):
    m = p if isinstance(p, dict) and "neg_lam" in p else f32_model(p)
    w = np.asarray(w, F)
    with np.errstate(all="ignore"):
        e = np.exp((m["neg_lam"] * (F(1) - w)).astype(np.float64)).astype(F)
        return (np.float64(m["Ron"]) / e.astype(np.float64)).astype(F)


def surface_u8(w, p=None, mode="state"):
    """The 8-bit surface frame of states w: "state" = uint8(w * 255f); "current" = uint8(clip(-3366 / log10(1 / R) - 306,
    0, 255)) in double on the float32 resistance."""
    w = np.asarray(w, F)
    if mode == "state":
        g = (w * F(255)).astype(np.float64)
    else:
        r = resistance_exp(w, p).astype(np.float64)
        g = -3366.0 / np.log10(1.0 / r) - 306.0
    return np.clip(g, 0.0, 255.0).astype(np.uint8)


def slice_bounds(t, slice_us):
    t = np.asarray(t, np.int64)
    return np.searchsorted(t, np.arange(t[0], t[-1] + slice_us, slice_us, dtype=np.int64))


def simulate(x, y, pol, t, H, W, version, polarity, slice_us, active_v, silent_v, p=None, dt=None,  # noqa: N803
             refractory_us=None, mid=None, n_slices=None, w0=None):
    """The slice loop.  Returns dict(w_final, resistances[, w_final_b, resistances_b]) with a snapshot after every slice whose
    index is a multiple of max(1, nslices // 100).  ``n_slices``: stop after that many slices (the snapshot cadence stays the
    whole stream's).  Scheme 1 pulses a pixel in every slice that holds an event of it (threshold 1)."""
    m = f32_model(p, dt)
    refr = REFRACTORY_US if refractory_us is None else int(refractory_us)
    x, y, pol, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(pol), np.asarray(t, np.int64)
    idx = slice_bounds(t, slice_us)
    total = len(idx) - 1
    every = max(1, total // 100)
    split = version == 2 and polarity == "split"
    narr = 2 if split else 1
    w = [np.full((H, W), m["wini"], F) if w0 is None else np.array(w0, F) for _ in range(narr)]
    next_ok = [np.zeros((H, W), np.int64) for _ in range(narr)]
    snaps = [[] for _ in range(narr)]
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
                        V[ys, xs] = act
                    else:
                        ok = next_ok[i][ys, xs] <= t[lo]
                        V[ys[ok], xs[ok]] = act
                        next_ok[i][ys[ok], xs[ok]] = t[hi - 1] + refr
            w[i] = update_state(w[i], V, m, mid=mid)
            if s % every == 0:
                snaps[i].append(resistance_exp(w[i], m))
    out = dict(w_final=w[0], resistances=np.array(snaps[0], F).reshape(-1, H, W))
    if split:
        out.update(w_final_b=w[1], resistances_b=np.array(snaps[1], F).reshape(-1, H, W))
    return out


def simulate_frames(imgs, dt=5e-4, n_sub=1000, th1=0.7, th2=1.5, p=None, dtype=np.float64):
    """The frame-driven loop in ``dtype`` (float64: the device's contract; np.longdouble: the sensitivity check).  Per frame
    pair the drive voltage from |a - b| * 256 through the piecewise map and the modulation, then n_sub Euler sub-steps of
    dw/dt = k * (V/v0 - 1)^alpha * (1 - w*s)^b (left to right), clipped to [0, 1].  Returns (w, resistances [n][H][W])."""
    p = DEFAULT if p is None else p
    T = dtype  # noqa: N806
    q = {k: T(p[k]) for k in KEYS}
    lam = np.log(T(p["Roff"]) / T(p["Ron"]))
    imgs = np.asarray(imgs, np.float64).astype(T)
    w = np.full(imgs.shape[1:], q["wini"], T)
    res = [q["Ron"] / np.exp(-lam * (1 - w))]
    dts = T(dt) / T(n_sub)
    with np.errstate(all="ignore"):
        for f in range(imgs.shape[0] - 1):
            d = np.abs(imgs[f] * 256 - imgs[f + 1] * 256)
            V = np.where(d > T(th1), (d + 4) * T(0.75), (d - T(5.5)) * T(0.6))  # noqa: N806
            V = np.where(V > 0, -(T(0.3) * V + 0), np.where(V < 0, -(3 * V + -3), T(0)))  # noqa: N806
            off, on = V < q["voff"], V > q["von"]
            ga = np.zeros(V.shape, T)
            for sel, v0, k, alpha in ((off, q["voff"], q["koff"], q["alphaoff"]), (on, q["von"], q["kon"], q["alphaon"])):
                a = V[sel] / v0 - 1
                ga[sel] = k * (a if alpha == 1 else np.power(a, alpha))
            s = np.where(off, q["soff"], q["son"])
            b = np.where(off, q["boff"], q["bon"])
            live = off | on
            for _ in range(n_sub):
                dw = np.where(live, ga * np.power(1 - w * s, b), T(0))
                nw = w + dw * dts
                w = np.where(nw < 0, T(0), np.where(nw > 1, T(1), nw))
            res.append(q["Ron"] / np.exp(-lam * (1 - w)))
    return w, np.array(res)
