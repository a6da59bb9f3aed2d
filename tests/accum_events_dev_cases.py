"""Event streams of the device-staging tests, shared by tests/test_accum_events_dev_cpu.py and
tests/test_accum_events_dev_gpu.py: seeded streams on a 64 x 48 sensor (W = 64 is a multiple of 16, so ``run_frames`` takes
the tile walk), each with the slice length it is cut at -- built once, shared, never modified.

  dense      6 000 events over 40 ms; a third of them on 24 pixels, so (pixel, slice) pairs repeat; p in {1, 0, -1}
  gaps       bursts with at least 3 empty slices between them; one slice holds a single event (its first and last event
             coincide), one holds several events of one time
  exact      the span is an exact multiple of slice_us: the events at the last time are dropped, bounds[-1] < n
  one        a single event: one bound, no slice
  same_time  every event at one time: one bound, no slice
  neg        times from -5 * 10^6
  sparse_us  slice_us = 1 over a 3 000 us span: more bounds than events
  blocky_N   N = 255, 256, 257, 1 023, 1 025, 70 001 events: the edges of a 256-event workgroup, and many workgroups
"""
import functools

import numpy as np

W, H = 64, 48
BLOCKY = (255, 256, 257, 1023, 1025, 70001)
SLICE_US = dict(dense=1000, gaps=1000, exact=1000, one=1000, same_time=1000, neg=1000, sparse_us=1,
                **{f"blocky_{n}": 1000 for n in BLOCKY})
CASES = tuple(SLICE_US)
STAGED = ("dense", "gaps", "exact")   # the cases the accumulators are compared on: at least 20 slices each


def _xyp(rng, n, hot=0):
    """n events anywhere on the sensor, the first `hot` of every three on 24 pixels."""
    x, y = rng.integers(0, W, n), rng.integers(0, H, n)
    if hot:
        px = rng.integers(0, 24, n)
        sel = rng.integers(0, 3, n) < hot
        x, y = np.where(sel, 8 + px % 6, x), np.where(sel, 10 + px // 6, y)
    return x.astype(np.int16), y.astype(np.int16), rng.choice(np.array([1, 0, -1], np.int8), n)


def _uniform(rng, n, t0, span):
    return np.sort(rng.integers(t0, t0 + span, n)).astype(np.int64)


def _build(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "dense":
        t = _uniform(rng, 6000, 0, 40_000)
        t[0], t[-1] = 0, 39_999
    elif name == "gaps":
        bursts = [_uniform(rng, 300, 0, 3000), _uniform(rng, 200, 7000, 2000), np.array([13_500]),
                  np.full(7, 17_250), _uniform(rng, 400, 21_000, 3000)]
        t = np.concatenate(bursts).astype(np.int64)
        t[0] = 0
    elif name == "exact":
        t = np.concatenate([[0], _uniform(rng, 900, 0, 20_000), np.full(5, 20_000)]).astype(np.int64)
    elif name == "one":
        t = np.array([123_456], np.int64)
    elif name == "same_time":
        t = np.full(300, 5000, np.int64)
    elif name == "neg":
        t = _uniform(rng, 2000, -5_000_000, 25_000)
    elif name == "sparse_us":
        t = _uniform(rng, 500, 10, 3000)
        t[0], t[-1] = 10, 3009
    else:
        t = _uniform(rng, int(name.split("_")[1]), 0, 40_000)
    x, y, p = _xyp(rng, len(t), hot=1 if name == "dense" else 0)
    for a in (x, y, p, t):
        a.setflags(write=False)
    return x, y, p, t


@functools.lru_cache(maxsize=None)
def stream(name):
    """-> (x int16, y int16, p int8, t int64 non-decreasing), read-only."""
    return _build(name)


def yardstick(name):
    """The bounds as the reference script forms them: searchsorted(t, arange(t[0], t[-1] + slice_us, slice_us))."""
    t, s = stream(name)[3], SLICE_US[name]
    return np.searchsorted(t, np.arange(t[0], t[-1] + s, s)).astype(np.int64)
