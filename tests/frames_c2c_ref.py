"""NumPy float64 restatement of the frame-driven run's cycle-to-cycle write noise (``nsof_accum_frames_f64_c2c*``,
``simulate_frames*(c2c=, trials=, first_pair=)``), shared by tests/test_frames_c2c_cpu.py and tests/test_frames_c2c_gpu.py --
and the cases the GPU file runs, the restatement of each computed once, shared, never modified.

The definition (include/nsof.h): for trial t, cell i = r * W + c and frame pair q = first_pair + f, V is the pair's drive
voltage as the noiseless run forms it; V < voff uses sigma_off, V > von sigma_on, anything else neither; xi is
``accum_c2c_ref.xi(seed, 0, t, i, q)``; u = 1.0 + float64(float32(sigma)) * float64(xi), f = max(0, u); one factor per pair, every
sub-step nw = w + (dwdt * f) * dts, then the clip.  The update is ``accum_params_ref.simulate_frames``'s, vectorised over
(trial, cell) with a device per (trial, cell).
"""
import functools

import numpy as np

import accum_c2c_ref as N  # noqa: N812
import accum_params_ref as R  # noqa: N812
from test_frames_maps_gpu import CLASSES, _class_planes, _labels

F = np.float32
DT, N_SUB = 5e-4, 50
THRESHOLDS = [(0.7, 1.5), (2.0, 1.5)]
GRIDS = [(1, 1), (4, 4), (13, 24)]
NOISE = dict(sigma_on=0.05, sigma_off=0.1, seed=0xF2A3E5000000C2C1)          # the main cases (b), (c)
CLAMP_NOISE = dict(sigma=1000.0, seed=77)                                    # (d)
ON_ONLY, OFF_ONLY = dict(sigma_on=0.2, seed=5), dict(sigma_off=0.2, seed=5)   # (e)
# the default device with both gains a tenth of the fitted ones: no state reaches 0 or 1 within one pair of the five frames, so
# a step that differs gives a state that differs (asserted in the CPU file)
QUIET = dict(R.DEFAULT, koff=R.DEFAULT["koff"] * 0.1, kon=R.DEFAULT["kon"] * 0.1)
# ... and without a power: alpha == 1 calls none, pow(x, 0) is 1 exactly
POW_FREE = dict(QUIET, alphaon=1, alphaoff=1, bon=0, boff=0)


def frames(grid):
    """The five frames of ``test_frames_dev_gpu._array_case`` (which also runs them on the device; the GPU file asserts
    they are these)."""
    rng = np.random.default_rng(grid[0] * 100 + grid[1])
    base = rng.random(grid)
    step = rng.choice([0.0, 0.002, 0.01, 0.3], size=(5,) + grid) * rng.standard_normal((5,) + grid)
    imgs = np.clip(base + step, 0.0, 1.0)
    imgs.setflags(write=False)
    return imgs


def voltage(a, b, th):
    """The drive voltage of a frame pair, as ``accum_params_ref.simulate_frames`` forms it."""
    d = np.abs(a * 256 - b * 256)
    V = np.where(d > th[0], (d + 4) * 0.75, (d - 5.5) * 0.6)  # noqa: N806
    return np.where(V > 0, -(0.3 * V + 0), np.where(V < 0, -(3 * V + -3), 0.0))


def simulate(imgs, trials, p=None, planes=None, noise=None, dt=DT, n_sub=N_SUB, th=THRESHOLDS[0], first_pair=0, w0=None):
    """The run of ``trials`` trials: ``p`` the scalars (``None``: the default device), ``planes`` a mapping key -> array
    broadcastable to [T][H][W] (a device per trial and cell), ``noise`` a ``c2c`` mapping as the tests write them (``None``: no
    noise), ``w0`` [T][H][W] the initial state instead of wini.  Returns a dict of read-only arrays, P = n - 1 pairs:
    ``w`` [P][T][H][W] the state after every pair, ``res`` [P + 1][T][H][W], ``off`` / ``on`` [P][T][H][W] the branch each pair
    took, ``xi`` float32 and ``u`` float64 [P][T][H][W] (u = 1 where no draw is made)."""
    p = R.DEFAULT if p is None else p
    imgs = np.asarray(imgs, np.float64)
    shape = (int(trials),) + imgs.shape[1:]
    q = {k: np.array(np.broadcast_to(np.asarray((planes or {}).get(k, p[k]), np.float64), shape)) for k in R.KEYS}
    sigma_on, sigma_off, seed = N.spreads(noise) if noise is not None else (F(0), F(0), 0)
    # (per element through the scalar logarithm accum_params_ref takes: NumPy's array logarithm may round another way)
    lam = np.array([np.log(v) for v in (q["Roff"] / q["Ron"]).ravel()]).reshape(shape)
    w = q["wini"].copy() if w0 is None else np.array(np.broadcast_to(np.asarray(w0, np.float64), shape))
    cell = np.arange(imgs[0].size).reshape(imgs.shape[1:])
    dts = np.float64(dt) / np.float64(n_sub)
    out = dict(w=[], res=[q["Ron"] / np.exp(-lam * (1 - w))], off=[], on=[], xi=[], u=[])
    with np.errstate(all="ignore"):
        for f in range(imgs.shape[0] - 1):
            V = np.broadcast_to(voltage(imgs[f], imgs[f + 1], th), shape)  # noqa: N806
            off, on = V < q["voff"], V > q["von"]
            ga = np.zeros(shape)
            for sel, v0, k, alpha in ((off, q["voff"], q["koff"], q["alphaoff"]), (on, q["von"], q["kon"], q["alphaon"])):
                a = V / v0 - 1
                # a ** alpha on the selected cells with a SCALAR exponent per distinct alpha, as accum_params_ref calls it:
                # NumPy's power with an array exponent takes another routine, which may round another way
                for v in np.unique(alpha[sel]):
                    if v != 1:
                        m = sel & (alpha == v)
                        a[m] = np.power(a[m], v)
                ga = np.where(sel, k * a, ga)
            s = np.where(off, q["soff"], q["son"])
            b = np.where(off, q["boff"], q["bon"])
            live = off | on
            x = np.stack([N.xi(seed, 0, t, cell, first_pair + f) for t in range(shape[0])])
            sigma = np.where(off, sigma_off, np.where(on, sigma_on, F(0))).astype(F)
            u = np.where(sigma != 0, 1.0 + sigma.astype(np.float64) * x.astype(np.float64), 1.0)
            fct = np.where(u < 0, 0.0, u)
            for _ in range(n_sub):
                dw = np.where(live, ga * np.power(1 - w * s, b), 0.0)
                nw = w + (dw * fct) * dts
                w = np.where(nw < 0, 0.0, np.where(nw > 1, 1.0, nw))
            out["w"].append(w)
            out["res"].append(q["Ron"] / np.exp(-lam * (1 - w)))
            for key, v in (("off", off), ("on", on), ("xi", x), ("u", u)):
                out[key].append(v)
    out = {k: np.array(v) for k, v in out.items()}
    for v in out.values():
        v.setflags(write=False)
    return out


def pow_free_planes(grid, trials=3):
    """Per-trial planes of koff, kon, voff and von around the pow-free device: a 10 % spread, signs kept."""
    rng = np.random.default_rng(1000 + grid[0])
    return {k: POW_FREE[k] * (1 + 0.1 * np.clip(rng.standard_normal((trials,) + grid), -3, 3)) for k in ("koff", "kon", "voff", "von")}


@functools.lru_cache(maxsize=None)
def pow_free_case(grid):
    """(b): T = 3 on the pow-free device with per-trial planes -> (frames, planes, the restatement)."""
    imgs, planes = frames(grid), pow_free_planes(grid)
    return imgs, planes, simulate(imgs, 3, POW_FREE, planes, NOISE)


CLASS_CASES = [((4, 4), 10), ((13, 24), 10), ((4, 4), 1000)]   # (c): grid, n_sub_steps


@functools.lru_cache(maxsize=None)
def class_case(grid, n_sub):
    """(c): T = 2, the three class devices as class planes -> (frames, planes, the noisy restatement, the noiseless one)."""
    imgs = frames(grid)
    planes = _class_planes(_labels(n_sub + grid[0], (2,) + grid))
    return (imgs, planes, simulate(imgs, 2, None, planes, NOISE, n_sub=n_sub), simulate(imgs, 2, None, planes, None, n_sub=n_sub))


@functools.lru_cache(maxsize=None)
def clamp_case():
    """(d): one pair on (13, 24), T = 5, sigma = 1000 on the default device."""
    imgs = frames((13, 24))[:2]
    return imgs, simulate(imgs, 5, None, None, CLAMP_NOISE)


def dead_zone_planes(grid):
    """von / voff planes that put every third cell's pair into the dead zone, whichever side its voltage lies on."""
    dead = (np.arange(grid[0] * grid[1]).reshape(grid) % 3) == 1
    return dict(von=np.where(dead, 1000.0, QUIET["von"]), voff=np.where(dead, -1000.0, QUIET["voff"]))


@functools.lru_cache(maxsize=None)
def direction_case(which):
    """(e): one pair on (13, 24), T = 2, noise on one branch only (``which``: "on" / "off"), the quiet device, every third cell
    in the dead zone -> (frames, planes, the noisy restatement, the noiseless one)."""
    imgs, planes = frames((13, 24))[:2], dead_zone_planes((13, 24))
    noise = ON_ONLY if which == "on" else OFF_ONLY
    return imgs, planes, simulate(imgs, 2, QUIET, planes, noise), simulate(imgs, 2, QUIET, planes, None)
