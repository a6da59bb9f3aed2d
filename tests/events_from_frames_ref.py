"""NumPy restatement of the level-crossing event generator (include/nsof.h, nsof_events_from_frames_*_dev; DESIGN.md
section 5.8): int64 throughout, vectorised per frame, the final order from np.lexsort.  It never calls the library."""
import numpy as np

UNITS = 256   # table units per grey level of the default (linear) response


def linear_lut():
    return np.arange(256, dtype=np.int64) * UNITS


def units(grey_levels):
    """A threshold in grey levels as table units, as the Python layer rounds it."""
    return int(round(UNITS * float(grey_levels)))


def events_from_frames_ref(frames, times, c_on, c_off, lut=None, ref=None, timestamps="linear", p_on=1, p_off=-1,
                           on_frame=None, on_stamps=None):
    """frames uint8 [n][H][W], times int64 [n]; c_on / c_off: table units, scalars or [H][W] planes; lut: 256 levels (None:
    256 * i); ref: None (zeros), "first" or an int [H][W] plane.  Returns a dict of x, y (int16), p (int8), t (int64),
    frame_bounds (int64 [n + 1]) and ref (int32 [H][W]).  The invariant -c_off < L[k] - r < c_on is asserted after every
    frame; on_frame(k, r, level) is called there too.  on_stamps(k, num, dt, den, t) is called per frame and polarity with the
    terms of the linear stamps t = T[k-1] + (num * dt) // den of its crossings (int64 arrays; dt an int)."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 3 and timestamps in ("frame", "linear")
    n, h, w = frames.shape
    times = np.asarray(times, np.int64)
    assert times.shape == (n,) and (np.diff(times) > 0).all()
    lut = linear_lut() if lut is None else np.asarray(lut, np.int64)
    con = np.broadcast_to(np.asarray(c_on, np.int64), (h, w)).reshape(-1)
    coff = np.broadcast_to(np.asarray(c_off, np.int64), (h, w)).reshape(-1)
    assert con.min() >= 1 and coff.min() >= 1
    level0 = lut[frames[0].reshape(-1)]
    if ref is None:
        r = np.zeros(h * w, np.int64)
    elif isinstance(ref, str):
        assert ref == "first"
        r = level0.copy()
    else:
        r = np.asarray(ref, np.int64).reshape(-1).copy()
    xs, ys, ps, ts, bounds = [], [], [], [], [0]
    a = level0   # L[k - 1]; unused for frame 0
    for k in range(n):
        b = lut[frames[k].reshape(-1)]
        d = b - r
        m_on = np.where(d >= con, d // con, 0)
        m_off = np.where(-d >= coff, (-d) // coff, 0)
        fx, fy, fpol, ft, fj = [], [], [], [], []
        for pol, m, c, sign in ((0, m_on, con, 1), (1, m_off, coff, -1)):
            idx = np.flatnonzero(m)
            if not idx.size:
                continue
            cnt = m[idx]
            pix = np.repeat(idx, cnt)
            j = np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt) + 1
            level = r[pix] + sign * j * c[pix]
            if timestamps == "frame" or k == 0:
                t = np.full(pix.size, times[k], np.int64)
            else:
                num, den = np.abs(level - a[pix]), np.abs(b[pix] - a[pix])
                assert (num > 0).all() and (den >= num).all()
                t = times[k - 1] + (num * (times[k] - times[k - 1])) // den
                assert (t >= times[k - 1]).all() and (t <= times[k]).all()
                if on_stamps is not None:
                    on_stamps(k, num, int(times[k] - times[k - 1]), den, t)
            fx.append(pix % w); fy.append(pix // w); fpol.append(np.full(pix.size, pol, np.int64)); ft.append(t); fj.append(j)
        r = r + m_on * con - m_off * coff
        assert ((b - r > -coff) & (b - r < con)).all(), f"invariant broken after frame {k}"
        if on_frame is not None:
            on_frame(k, r.reshape(h, w), b.reshape(h, w))
        a = b
        if fx:
            fx, fy, fpol, ft, fj = (np.concatenate(v) for v in (fx, fy, fpol, ft, fj))
            order = np.lexsort((fj, fx, fy, fpol, ft))   # the last key is the primary one: (t, polarity, y, x, j)
            xs.append(fx[order]); ys.append(fy[order]); ts.append(ft[order])
            ps.append(np.where(fpol[order] == 0, p_on, p_off))
        bounds.append(bounds[-1] + len(fx))
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)  # noqa: E731
    return dict(x=cat(xs, np.int16), y=cat(ys, np.int16), p=cat(ps, np.int8), t=cat(ts, np.int64),
                frame_bounds=np.asarray(bounds, np.int64), ref=r.reshape(h, w).astype(np.int32))


def log_lut(eps=1.0):
    """A host-built logarithmic response with the linear table's range."""
    i = np.arange(256, dtype=np.float64)
    v = (np.log(i + eps) - np.log(eps)) / (np.log(255.0 + eps) - np.log(eps))
    return np.rint(UNITS * 255 * v).astype(np.int64)


def drifting_texture(n, h, w, seed=7):
    """n frames of a texture drifting by consecutive make_pair shifts (host, uint8 [n][h][w])."""
    from nsof import synth
    frames = synth.make_sequence(seed, n, h, w)
    assert np.array_equal(frames[n - 1], synth.make_pair(seed, h, w, shift=(2.5 * (n - 1), -1.25 * (n - 1)), rot_deg=0.2 * (n - 1))[1])
    return frames
