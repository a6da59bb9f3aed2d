"""Scheme 1's event-count threshold (THETA_EVENTS) restated in NumPy: ``accum_params_ref.simulate`` with the count test, and
the stream filter that defines what a threshold run is -- the theta == 1 run on the stream without the events of every
(pixel, slice) cell that holds fewer than theta events.  Polarity is not read: every event counts."""
import numpy as np

import accum_params_ref as R

F = np.float32


def cell_counts(x, y, bounds, W):  # noqa: N803
    """Per event of [bounds[0], bounds[-1]): its slice and the number of events in its (pixel, slice) cell."""
    bounds = np.asarray(bounds, np.int64)
    e = np.arange(bounds[0], bounds[-1])
    sl = np.searchsorted(bounds, e, side="right") - 1          # the largest s with bounds[s] <= e (empty slices repeat a bound)
    x, y = np.asarray(x, np.int64)[e], np.asarray(y, np.int64)[e]
    key = (sl * (int(y.max(initial=0)) + 1) + y) * int(W) + x
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    return sl, cnt[inv.reshape(-1)]


def filter_stream(x, y, p, t, bounds, theta, W):  # noqa: N803
    """-> ((x, y, p, t), bounds) of the same stream without the events of cells that hold fewer than ``theta`` events: the
    same slices, their bounds re-indexed."""
    bounds = np.asarray(bounds, np.int64)
    sl, c = cell_counts(x, y, bounds, W)
    keep = c >= theta
    lo, hi = int(bounds[0]), int(bounds[-1])
    ev = tuple(np.ascontiguousarray(np.asarray(a)[lo:hi][keep]) for a in (x, y, p, t))
    per_slice = np.bincount(sl[keep], minlength=len(bounds) - 1)
    return ev, np.concatenate([[0], np.cumsum(per_slice)]).astype(np.int64)


def simulate(x, y, t, H, W, slice_us, active_v, silent_v, theta, p=None, dt=None):  # noqa: N803
    """``accum_params_ref.simulate(version=1)`` with ``bincount_2d >= theta`` as the pulse test (event_mem_sim.py:208-217).
    Returns dict(w_final, resistances) with a snapshot after every slice whose index is a multiple of max(1, nslices // 100)."""
    m = R.f32_model(p, dt)
    x, y, t = np.asarray(x, np.int64), np.asarray(y, np.int64), np.asarray(t, np.int64)
    idx = R.slice_bounds(t, slice_us)
    total = len(idx) - 1
    every = max(1, total // 100)
    w = np.full((H, W), m["wini"], F)
    snaps = []
    for s in range(total):
        lo, hi = int(idx[s]), int(idx[s + 1])
        counts = np.zeros((H, W), np.int64)
        np.add.at(counts, (y[lo:hi], x[lo:hi]), 1)
        V = np.full((H, W), F(silent_v), F)  # noqa: N806
        V[counts >= theta] = F(active_v)
        w = R.update_state(w, V, m)
        if s % every == 0:
            snaps.append(R.resistance_exp(w, m))
    return dict(w_final=w, resistances=np.array(snaps, F).reshape(-1, H, W))
