"""NumPy / Python-int restatement of the event generator's sensor model (include/nsof.h,
nsof_events_from_frames_sensor_*_dev): the level crossings of tests/events_from_frames_ref.py, one
Philox block of noise per pixel and interval, and the refractory walk, int64 throughout.  It never calls the library.

Per frame k of a call every pixel has candidates: its m signal crossings with their stamps (r moves by m thresholds whether
or not they survive) and, for k >= 1, up to two noise events from the block of (pixel, first_frame + k).  They are walked in
the order (t, signal before ON noise before OFF noise, crossing); one is emitted iff t >= t_ok, and then t_ok = t +
refractory_us.  The frame's survivors are ordered by (t, ON before OFF, y, x, j), a noise event being the last j of its
polarity.  The walk is always made here -- with refractory_us = 0 and no t_ok it drops nothing, which the tests check
against events_from_frames_ref.
"""
import numpy as np

from accum_c2c_ref import philox4x32_10
from events_from_frames_ref import linear_lut

NEVER = np.iinfo(np.int64).min      # t_ok of a pixel that has not fired
NOISE_WORD = 0x4E534546             # the fourth counter word of a noise block
U = np.uint64


def rate_q(hz):
    """A rate in Hz in the model's units of 2^-32 per microsecond, as the Python layer rounds it."""
    return int(round(float(hz) * 4294967296.0 / 1e6))


def noise_words(seed, pixel, frame):
    """c0..c3 (uint64 arrays below 2^32) of the noise block of (seed, pixel, absolute frame index), broadcast over pixel."""
    f = int(frame)
    return philox4x32_10(np.asarray(pixel, U), U(f & 0xFFFFFFFF), U(f >> 32), U(NOISE_WORD), int(seed) & 0xFFFFFFFF, int(seed) >> 32)


def noise_candidates(seed, npx, frame, delta, rate_on, rate_off):
    """The noise of all pixels in an interval of delta microseconds before absolute frame `frame`: (ON exists, ON offset, OFF
    exists, OFF offset), offsets from the interval's start as int64.  rate_*: uint64 arrays [npx] of rate units."""
    c0, c1, c2, c3 = noise_words(seed, np.arange(npx), frame)
    top = U(0xFFFFFFFF)
    p_on, p_off = np.minimum(top, rate_on * U(delta)), np.minimum(top, rate_off * U(delta))   # below 2^32 * 2^31: no overflow
    return c0 < p_on, ((c2 * U(delta)) >> U(32)).astype(np.int64), c1 < p_off, ((c3 * U(delta)) >> U(32)).astype(np.int64)


def events_sensor_ref(frames, times, c_on, c_off, lut=None, ref=None, timestamps="linear", p_on=1, p_off=-1, refractory_us=0,
                      seed=0, rate_on=0, rate_off=0, t_ok=None, first_frame=0, counter_of=None):
    """frames uint8 [n][H][W], times int64 [n]; c_on / c_off: table units, scalars or [H][W]; rate_on / rate_off: rate
    units (rate_q), scalars or [H][W]; ref: None, "first" or an int [H][W] plane; t_ok: None or an int64 [H][W] plane.
    Returns a dict of x, y (int16), p (int8), t (int64), frame_bounds (int64 [n + 1]), ref (int32 [H][W]), t_ok (int64
    [H][W]) and noise (int64 [2]: the ON and OFF noise candidates drawn, before the walk).  counter_of(first_frame, k): the
    frame index the noise block of frame k is drawn for (None: the model's first_frame + k; a test of the counter's carry
    states a wrong generator with it).  t_ok = t + refractory_us must stay an int64, as the entries require."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 3 and timestamps in ("frame", "linear")
    n, h, w = frames.shape
    npx = h * w
    times = np.asarray(times, np.int64)
    assert times.shape == (n,) and (np.diff(times) > 0).all() and (np.diff(times) < 1 << 31).all()
    assert 0 <= refractory_us < 1 << 31 and first_frame >= 0
    assert refractory_us == 0 or int(times[-1]) <= np.iinfo(np.int64).max - refractory_us, "t_ok would pass the int64 range"
    lut = linear_lut() if lut is None else np.asarray(lut, np.int64)
    con = np.broadcast_to(np.asarray(c_on, np.int64), (h, w)).reshape(-1)
    coff = np.broadcast_to(np.asarray(c_off, np.int64), (h, w)).reshape(-1)
    ron = np.broadcast_to(np.asarray(rate_on, U), (h, w)).reshape(-1)
    roff = np.broadcast_to(np.asarray(rate_off, U), (h, w)).reshape(-1)
    assert con.min() >= 1 and coff.min() >= 1 and ron.max() < 1 << 32 and roff.max() < 1 << 32
    level0 = lut[frames[0].reshape(-1)]
    if ref is None:
        r = np.zeros(npx, np.int64)
    elif isinstance(ref, str):
        assert ref == "first"
        r = level0.copy()
    else:
        r = np.asarray(ref, np.int64).reshape(-1).copy()
    tok = (np.full(npx, NEVER, np.int64) if t_ok is None else np.asarray(t_ok, np.int64).reshape(-1)).tolist()   # Python ints
    xs, ys, ps, ts, bounds = [], [], [], [], [0]
    drawn = np.zeros(2, np.int64)
    a = level0   # L[k - 1]; unused for frame 0
    for k in range(n):
        b = lut[frames[k].reshape(-1)]
        d = b - r
        m_on = np.where(d >= con, d // con, 0)
        m_off = np.where(-d >= coff, (-d) // coff, 0)
        same = timestamps == "frame" or k == 0
        # the candidates of the frame: pixel, polarity (0 ON, 1 OFF), kind (0 signal, 1 ON noise, 2 OFF noise), j, t
        cp, cpol, ckind, cj, ct = [], [], [], [], []
        for pol, m, c, sign in ((0, m_on, con, 1), (1, m_off, coff, -1)):
            idx = np.flatnonzero(m)
            if not idx.size:
                continue
            cnt = m[idx]
            pix = np.repeat(idx, cnt)
            j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + 1
            if same:
                t = np.full(pix.size, times[k], np.int64)
            else:
                level = r[pix] + sign * j * c[pix]
                num, den = np.abs(level - a[pix]), np.abs(b[pix] - a[pix])
                assert (num > 0).all() and (den >= num).all()
                t = times[k - 1] + (num * (times[k] - times[k - 1])) // den
            cp.append(pix); cpol.append(np.full(pix.size, pol, np.int64)); ckind.append(np.zeros(pix.size, np.int64)); cj.append(j); ct.append(t)
        if k >= 1:
            delta = int(times[k] - times[k - 1])
            has_on, o_on, has_off, o_off = noise_candidates(seed, npx, first_frame + k if counter_of is None else counter_of(first_frame, k),
                                                           delta, ron, roff)
            for pol, has, off, m in ((0, has_on, o_on, m_on), (1, has_off, o_off, m_off)):
                idx = np.flatnonzero(has)
                drawn[pol] += idx.size
                assert (off >= 0).all() and (off < delta).all()
                t = np.full(idx.size, times[k], np.int64) if same else times[k - 1] + off[idx]
                cp.append(idx); cpol.append(np.full(idx.size, pol, np.int64)); ckind.append(np.full(idx.size, 1 + pol, np.int64))
                cj.append(m[idx] + 1); ct.append(t)   # after every signal crossing of its polarity
        r = r + m_on * con - m_off * coff   # whether or not the crossings survive
        assert ((b - r > -coff) & (b - r < con)).all(), f"invariant broken after frame {k}"
        a = b
        count = 0
        if cp:
            cp, cpol, ckind, cj, ct = (np.concatenate(v) for v in (cp, cpol, ckind, cj, ct))
            walk = np.lexsort((cj, ckind, ct, cp))   # per pixel: (t, kind, crossing)
            keep = np.zeros(cp.size, bool)
            for i, pix, t in zip(walk.tolist(), cp[walk].tolist(), ct[walk].tolist()):
                if t >= tok[pix]:
                    keep[i] = True
                    tok[pix] = t + refractory_us
            cp, cpol, cj, ct = cp[keep], cpol[keep], cj[keep], ct[keep]
            order = np.lexsort((cj, cp % w, cp // w, cpol, ct))   # (t, polarity, y, x, j)
            xs.append((cp % w)[order]); ys.append((cp // w)[order]); ts.append(ct[order])
            ps.append(np.where(cpol[order] == 0, p_on, p_off))
            count = int(keep.sum())
        bounds.append(bounds[-1] + count)
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)  # noqa: E731
    return dict(x=cat(xs, np.int16), y=cat(ys, np.int16), p=cat(ps, np.int8), t=cat(ts, np.int64),
                frame_bounds=np.asarray(bounds, np.int64), ref=r.reshape(h, w).astype(np.int32),
                t_ok=np.array(tok, np.int64).reshape(h, w), noise=drawn)
