"""The background-activity filter restated for the tests, three ways:

``denoise_walk``      the rule as it is written: a sequential walk over the stream in NumPy int64.
``denoise_walk_int``  the same walk in Python ints, which cannot wrap: the check of the int64 walk's own arithmetic.
``denoise_sorted``    the parallel formulation the kernels follow -- a stable sort of (channel, pixel) keys, and per event and
                      neighbour the last entry of the neighbour's segment with a stream index below the event's -- in NumPy.

All take the stream (``x, y`` int16, ``p`` int8, ``t`` int64, ``t`` non-decreasing), the sensor's ``H, W``, the filter's
parameters and an optional ``last`` (int64 ``[C][H][W]``) and return ``(keep uint8 [N], last int64 [C][H][W])``.
``denoise_result`` adds what the device call returns besides: the kept stream, ``n_kept`` and the kept stream's bounds.
"""
import numpy as np

NEVER = np.iinfo(np.int64).min
I64_MAX = np.iinfo(np.int64).max


def _state(last, c, H, W):  # noqa: N803
    if last is None:
        return np.full((c, H, W), NEVER, np.int64)
    last = np.asarray(last)
    assert last.dtype == np.int64 and last.shape == (c, H, W)
    return last.copy()


def denoise_walk(x, y, p, t, H, W, dt_us, radius=1, min_support=1, same_polarity=False, include_self=False, last=None):  # noqa: N803
    c = 2 if same_polarity else 1
    last = _state(last, c, H, W)
    keep = np.zeros(len(x), np.uint8)
    floor = np.int64(NEVER + 1)
    edge = np.int64(NEVER + 1 + dt_us)   # below it t - dt_us would pass the floor (or wrap)
    dt = np.int64(dt_us)
    for i in range(len(x)):
        xi, yi, ti = int(x[i]), int(y[i]), t[i]
        ch = 0 if not same_polarity or p[i] > 0 else 1
        lo = floor if ti < edge else ti - dt
        win = last[ch, max(yi - radius, 0):yi + radius + 1, max(xi - radius, 0):xi + radius + 1]
        support = int(np.count_nonzero(win >= lo))
        if not include_self and last[ch, yi, xi] >= lo:
            support -= 1
        keep[i] = support >= min_support
        last[ch, yi, xi] = ti
    return keep, last


def denoise_walk_int(x, y, p, t, H, W, dt_us, radius=1, min_support=1, same_polarity=False, include_self=False, last=None):  # noqa: N803
    c = 2 if same_polarity else 1
    state = [int(v) for v in _state(last, c, H, W).ravel()]
    never = int(NEVER)
    keep = np.zeros(len(x), np.uint8)
    xs, ys, ps, ts = (v.tolist() for v in (x, y, p, t))
    for i in range(len(xs)):
        xi, yi, ti = xs[i], ys[i], ts[i]
        base = (H * W if same_polarity and ps[i] <= 0 else 0)
        lo = max(ti - dt_us, never + 1)
        support = 0
        for ny in range(max(yi - radius, 0), min(yi + radius, H - 1) + 1):
            for nx in range(max(xi - radius, 0), min(xi + radius, W - 1) + 1):
                if (include_self or ny != yi or nx != xi) and state[base + ny * W + nx] >= lo:
                    support += 1
        keep[i] = support >= min_support
        state[base + yi * W + xi] = ti
    return keep, np.array(state, np.int64).reshape(c, H, W)


def denoise_sorted(x, y, p, t, H, W, dt_us, radius=1, min_support=1, same_polarity=False, include_self=False, last=None):  # noqa: N803
    c = 2 if same_polarity else 1
    incoming = _state(last, c, H, W).ravel()
    n = len(x)
    i = np.arange(n, dtype=np.int64)
    xs, ys = x.astype(np.int64), y.astype(np.int64)
    base = np.where(p <= 0, H * W, 0).astype(np.int64) if same_polarity else np.zeros(n, np.int64)
    key = base + ys * W + xs
    order = np.argsort(key, kind="stable")
    words = key[order] << 32 | order   # ascending by (key, stream index)
    with np.errstate(over="ignore"):
        lo = np.where(t < NEVER + 1 + dt_us, NEVER + 1, t - np.int64(dt_us))
    support = np.zeros(n, np.int64)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0 and not include_self:
                continue
            ny, nx = ys + dy, xs + dx
            inside = (ny >= 0) & (ny < H) & (nx >= 0) & (nx < W)
            nkey = np.where(inside, base + ny * W + nx, 0)
            pos = np.searchsorted(words, nkey << 32 | i, side="left")   # the entries below (neighbour's key, i)
            prev = words[np.maximum(pos - 1, 0)] if n else words
            hit = (pos > 0) & (prev >> 32 == nkey)
            seen = np.where(hit, t[prev & 0xffffffff] if n else t, incoming[nkey])
            support += inside & (seen >= lo)
    out = incoming.copy()
    if n:
        ends = np.flatnonzero(np.append(np.diff(key[order]) != 0, True))   # the last entry of every segment
        out[key[order][ends]] = t[order[ends]]
    return (support >= min_support).astype(np.uint8), out.reshape(c, H, W)


def denoise_result(x, y, p, t, keep, last, bounds=None):
    """What ``events_denoise_dev`` returns for a keep mask: the kept stream, ``n_kept``, the kept counts before ``bounds``."""
    k = keep.astype(bool)
    before = np.concatenate([[0], np.cumsum(keep, dtype=np.int64)])
    return dict(x=x[k], y=y[k], p=p[k], t=t[k], keep=keep, n_kept=int(k.sum()), last=last,
                bounds=None if bounds is None else before[np.asarray(bounds, np.int64)])
