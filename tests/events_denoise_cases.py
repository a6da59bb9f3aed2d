"""The inputs the background-activity filter is tested on, shared by tests/test_events_denoise_cpu.py (the restatements
against each other, the keep shares) and tests/test_events_denoise_gpu.py (the device against the restatement).  A case:
the stream, the sensor, the filter's arguments, an optional incoming ``last``, bounds, and the cuts at which it is also run in
two calls.  ``want(name)`` is the sequential walk's result, computed once per session and read-only.
"""
import functools
import os

import numpy as np

from events_denoise_ref import I64_MAX, NEVER, denoise_result, denoise_walk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {}


def _add(name, x, y, p, t, hw, kw, last=None, cuts=(), share=None, bounds=None):
    """share: the (lowest, highest) share of events the walk must keep (tests/test_events_denoise_cpu.py asserts it)."""
    x, y, p, t = np.asarray(x, np.int16), np.asarray(y, np.int16), np.asarray(p, np.int8), np.asarray(t, np.int64)
    n = len(x)
    assert len(y) == len(p) == len(t) == n and (np.diff(t.astype(object)) >= 0).all(), name
    if bounds is None:
        bounds = [0, n // 4, n // 4, n // 2, n - n // 5, n, n]
    case = dict(x=x, y=y, p=p, t=t, hw=hw, kw=kw, last=last, cuts=tuple(cuts), share=share, bounds=np.asarray(bounds, np.int64))
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    assert name not in CASES
    CASES[name] = case


def _tie_cut(t):
    """An index inside a run of equal t (not at its start): the cut falls between two events of one time stamp."""
    same = np.flatnonzero(np.diff(t) == 0)
    assert len(same), "no ties"
    return int(same[len(same) // 2]) + 1


def _random(name, H, W, n, t_span, seed, share=(0.05, 0.95), **kw):  # noqa: N803
    """n events at uniformly random pixels and polarities, times drawn from [0, t_span) and sorted: with t_span < n there are ties."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, t_span, n)).astype(np.int64)
    _add(name, rng.integers(0, W, n), rng.integers(0, H, n), rng.choice([-1, 1], n), t, (H, W), kw, cuts=(n // 3, _tie_cut(t)), share=share)


# ---- random streams with ties -------------------------------------------------------------------------------------------
_random("5x7", 5, 7, 3000, 2500, 1, dt_us=3)
_random("1x1-self", 1, 1, 200, 150, 2, dt_us=0, include_self=True)
_random("1x1-no-self", 1, 1, 200, 150, 2, share=(0.0, 0.0), dt_us=100, include_self=False)   # no neighbour: nothing is kept
_random("1x9-r2", 1, 9, 1500, 1200, 3, dt_us=3, radius=2, min_support=2, same_polarity=True)
_random("9x4-dt0", 9, 4, 2000, 100, 4, dt_us=0, same_polarity=True, include_self=True)
# 274 workgroups of 256 events: the scan of their counts carries from its first 256 entries into the second chunk.  (Two channels
# of 33 x 65 are 4290 keys, 13 bits of the sort; more than 16 key bits come from 300 x 301 -- with as many workgroups in
# "300x301-many" -- and from the two 32767-long sensors.)
_random("33x65", 33, 65, 70001, 60000, 5, dt_us=40, same_polarity=True)
# The exact chunk boundaries: one full chunk of 256 events and a second chunk of one event; a table of exactly 256 chunk counts
# (one step of the scan, no carry) and a 257th count, the carry into a step of one entry -- which must not be zero.
_random("5x7-256", 5, 7, 256, 213, 21, dt_us=3)
_random("5x7-257", 5, 7, 257, 214, 22, dt_us=3)
_random("33x65-65536", 33, 65, 65536, 56000, 23, dt_us=150, same_polarity=True)
_random("33x65-65537", 33, 65, 65537, 56000, 24, dt_us=150, same_polarity=True)


def _last_is_kept(name):
    """The case's last event has an earlier event of its polarity within dt_us in its window of radius 1 (min_support is 1)."""
    c = CASES[name]
    x, y, p, t = (c[k].astype(np.int64) for k in "xypt")
    near = (np.abs(x[:-1] - x[-1]) <= 1) & (np.abs(y[:-1] - y[-1]) <= 1) & ((x[:-1] != x[-1]) | (y[:-1] != y[-1]))
    return bool((near & ((p[:-1] > 0) == (p[-1] > 0)) & (t[:-1] >= t[-1] - c["kw"]["dt_us"])).any())


assert _last_is_kept("33x65-65537")
_random("5x5-r2-m9",5, 5, 4000, 300, 6, dt_us=3, radius=2, min_support=9, include_self=True)   # a corner's whole window, self included


def _hot_pixel():
    """20 000 events at one pixel of 8 x 8 among 2000 elsewhere: a segment far longer than a wave."""
    rng = np.random.default_rng(7)
    n = 22000
    hot = np.zeros(n, bool)
    hot[rng.choice(n, 20000, replace=False)] = True
    x, y = np.where(hot, 3, rng.integers(0, 8, n)), np.where(hot, 4, rng.integers(0, 8, n))
    t = np.sort(rng.integers(0, 200000, n)).astype(np.int64)
    _add("hot-pixel", x, y, rng.choice([-1, 1], n), t, (8, 8), dict(dt_us=60, min_support=1), cuts=(n // 3,), share=(0.05, 0.95))
    _add("hot-pixel-self", x, y, rng.choice([-1, 1], n), t, (8, 8), dict(dt_us=8, include_self=True, same_polarity=True), cuts=(n // 2,),
         share=(0.05, 0.95))


def _borders():
    """Events on the border and in the corners of 7 x 9 only, radius 2: every window is clipped, on one side or two."""
    rng = np.random.default_rng(8)
    ring = [(yy, xx) for yy in range(7) for xx in range(9) if yy in (0, 6) or xx in (0, 8)]
    n = 2500
    pick = rng.integers(0, len(ring), n)
    y, x = np.array(ring)[pick].T
    t = np.sort(rng.integers(0, 2000, n)).astype(np.int64)
    _add("borders-r2", x, y, rng.choice([-1, 1], n), t, (7, 9), dict(dt_us=4, radius=2, min_support=2), cuts=(n // 3, _tie_cut(t)),
         share=(0.05, 0.95))


def _wide_tall():
    """32767 x 1 and 1 x 32767 with 50 events in three clusters, the last coordinate included."""
    rng = np.random.default_rng(9)
    pos = np.concatenate([rng.integers(0, 4, 17), rng.integers(16000, 16004, 16), rng.integers(32763, 32767, 17)])
    pos = pos[rng.permutation(50)]
    pos[7] = 32766
    t = np.sort(rng.integers(0, 400, 50)).astype(np.int64)
    p = rng.choice([-1, 1], 50)
    zero = np.zeros(50, np.int64)
    _add("wide", pos, zero, p, t, (1, 32767), dict(dt_us=60), cuts=(17,), share=(0.05, 0.95))
    _add("tall", zero, pos, p, t, (32767, 1), dict(dt_us=60, radius=2, same_polarity=True), cuts=(17,), share=(0.05, 0.95))


def _large_plane():
    """300 x 301 with both channels: 180 600 keys, 18 bits of the sort.  Events in a few patches and in the last corner; once
    6000 of them, once 70 001: the 18-bit sort together with 274 workgroups and the carry of the chunk scan."""
    for name, n, t_span, dt_us in (("300x301", 6000, 5000, 150), ("300x301-many", 70001, 60000, 150)):
        rng = np.random.default_rng(10)
        cy, cx = rng.choice([3, 150, 296], n), rng.choice([2, 151, 297], n)
        y, x = cy + rng.integers(-3, 4, n), cx + rng.integers(-2, 4, n)
        y[:5], x[:5] = 299, 300
        t = np.sort(rng.integers(0, t_span, n)).astype(np.int64)
        _add(name, x, y, rng.choice([-1, 1], n), t, (300, 301), dict(dt_us=dt_us, same_polarity=True, min_support=2),
             cuts=(n // 3, _tie_cut(t)), share=(0.05, 0.95))


def _extreme_times():
    """t from INT64_MIN upward and up to INT64_MAX on 3 x 3: lo = t - dt_us must saturate at INT64_MIN + 1, not wrap; an event
    at INT64_MIN itself leaves its pixel at `never`."""
    rng = np.random.default_rng(11)
    low = NEVER + np.array([0, 0, 1, 1, 2, 5, 5, 900, 1000, 1001, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 3], dtype=object)
    mid = np.array([-5, -1, 0, 0, 7, 2 ** 31 + 2, 2 ** 31 + 5], dtype=object)
    high = I64_MAX - np.array([2 ** 31 + 9, 2 ** 31, 2 ** 31 - 1, 50, 49, 3, 1, 0, 0], dtype=object)
    t = np.array([int(v) for v in np.concatenate([low, mid, high])], np.int64)
    n = len(t)
    x, y, p = rng.integers(0, 3, n), rng.integers(0, 3, n), rng.choice([-1, 1], n)
    for name, kw in (("extreme-t-dt-max", dict(dt_us=2 ** 31 - 1)), ("extreme-t-dt-3", dict(dt_us=3, include_self=True)),
                     ("extreme-t-dt-0", dict(dt_us=0, include_self=True, radius=2))):
        _add(name, x, y, p, t, (3, 3), kw, cuts=(2, 14, n - 1))


def _given_last():
    """An incoming state that holds `never`, values above every t of the stream, and INT64_MAX."""
    rng = np.random.default_rng(12)
    n = 600
    t = np.sort(rng.integers(1000, 1400, n)).astype(np.int64)
    for name, c, kw in (("last-1", 1, dict(dt_us=2)), ("last-2", 2, dict(dt_us=2, same_polarity=True, include_self=True))):
        last = rng.integers(900, 1100, (c, 4, 4)).astype(np.int64)
        last[:, 0, :] = NEVER
        last[:, 1, 1] = 5000
        last[:, 2, 3] = I64_MAX
        last[0, 3, 0] = NEVER + 1
        _add(name, rng.integers(0, 4, n), rng.integers(0, 4, n), rng.choice([-1, 1], n), t, (4, 4), kw, last=last, cuts=(n // 3, _tie_cut(t)),
             share=(0.05, 0.95))
    none = np.zeros(0, np.int64)
    _add("n0", none, none, none, none, (3, 5), dict(dt_us=10), bounds=[0, 0])
    _add("n0-last", none, none, none, none, (3, 5), dict(dt_us=10, same_polarity=True), last=rng.integers(0, 9, (2, 3, 5)).astype(np.int64), bounds=[])
    _add("n1", [2], [1], [1], [77], (3, 5), dict(dt_us=10), cuts=(0, 1))
    _add("n1-self", [2], [1], [-1], [77], (3, 5), dict(dt_us=10, include_self=True, same_polarity=True),
         last=np.full((2, 3, 5), 70, np.int64), cuts=(1,))


def _generator_stream():
    """The generator's own stream (tests/golden/synth_events.npz: a box moving over 60 x 90), as it is and with noise events
    spliced in on the host: uniformly random pixels and times, merged stably by t."""
    g = np.load(os.path.join(GOLDEN, "synth_events.npz"))
    x, y, p, t = (g[f"small_{k}"] for k in "xypt")
    n = len(x)
    _add("box", x, y, p, t, (60, 90), dict(dt_us=250), cuts=(n // 3, _tie_cut(t)))   # not random, and clean: 95.3 % are kept
    rng = np.random.default_rng(13)
    m = 1800
    xa, ya = np.concatenate([x, rng.integers(0, 90, m)]), np.concatenate([y, rng.integers(0, 60, m)])
    pa, ta = np.concatenate([p, rng.choice([-1, 1], m)]), np.concatenate([t, rng.integers(0, int(t[-1]) + 1, m)])
    order = np.argsort(ta, kind="stable")
    _add("box-noise", xa[order], ya[order], pa[order], ta[order], (60, 90), dict(dt_us=1500, same_polarity=True, min_support=2),
         cuts=((n + m) // 3, _tie_cut(ta[order])), share=(0.05, 0.95))
    noise = order >= n   # in the merged order: which events are noise
    CASES["box-noise"]["is_noise"] = noise


_hot_pixel()
_borders()
_wide_tall()
_large_plane()
_extreme_times()
_given_last()
_generator_stream()

NAMES = tuple(CASES)


def stream(name, lo=0, hi=None):
    c = CASES[name]
    return tuple(c[k][lo:hi] for k in "xypt")


@functools.lru_cache(maxsize=None)
def walk(name, lo=0, hi=None, carried=None):
    """(keep, last) of the sequential walk over events [lo, hi) of the case; carried: the cut whose first call's state comes in."""
    c = CASES[name]
    last = c["last"] if carried is None else walk(name, 0, carried)[1]
    keep, out = denoise_walk(*stream(name, lo, hi), *c["hw"], last=last, **c["kw"])
    keep.setflags(write=False)
    out.setflags(write=False)
    return keep, out


def want(name):
    """What events_denoise_dev must return for the whole case with the case's bounds."""
    keep, last = walk(name)
    return denoise_result(*stream(name), keep, last, CASES[name]["bounds"])
