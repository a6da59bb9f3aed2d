"""Inputs of the event generator's limit tests, shared by tests/test_events_limits_cpu.py and tests/test_events_limits_gpu.py:
the corner of the argument space that csrc/events_from_frames.hip has arithmetic for and the other event tests do not reach.
Pure NumPy, a fixed seed per case.  cases() yields (name, frames, times, the keyword arguments of events_from_frames_dev, the
restatement's); restatement(name) is the restatement's run of a case (tests/events_from_frames_ref.py for the plain entries,
tests/events_sensor_ref.py for the sensor entries), computed once, shared, never modified; PRECONDITIONS[group](name) asserts,
on the restatement alone, what makes the case a limit case.

  A  coordinates up to 32766 (the 15-bit fields of the packed (x, y, polarity) word) and a frame of 353 workgroups, where the
     scan of a table row carries between its 256-entry chunks
  B  negative times and a linear-stamp key t - T[0] of 33 bits
  C  stamp products num * dt beyond 2^53, where a quotient formed in double is a wrong one
  D  a reference plane nobody produced: |L - r| of 2^31 and more
  E  the noise counter's carry from its second word into its third
  F  both sides of the 2^20 crossings a thread walks one by one
  G  times at the top of the int64 range: t_ok = t + refractory_us up to INT64_MAX exactly

A device argument `ref` is a host int32 plane here; the GPU file uploads it.
"""
import functools

import numpy as np

from events_from_frames_ref import drifting_texture, events_from_frames_ref
from events_sensor_ref import events_sensor_ref, rate_q

INT64_MAX = int(np.iinfo(np.int64).max)
MODES = ("frame", "linear")
SENSOR_KEYS = ("refractory_us", "seed", "rate_on", "rate_off", "first_frame", "t_ok")

T_SHORT = np.array([0, 1000, 5000], np.int64)
T0 = -5_000_000_000
T_WIDE = T0 + np.array([0, 2_000_000_000, 3_500_000_000, 5_200_000_000], np.int64)   # gaps below 2^31; the last straddles T0 + 2^32
T_SENSOR = np.array([5, 33338, 50005, 120005, 121005, 200005], np.int64)   # TIMES[:6] of tests/test_events_sensor_gpu.py
STEEP = np.arange(256, dtype=np.int64) << 22       # a response table over [0, 2^30)
C_STEEP = 3 * (1 << 22) + 1                        # table units: m <= 85 per step on STEEP
C_EXACT = (1 << 20) + 7                            # odd; EXACT's steps are whole multiples of it
EXACT = np.arange(256, dtype=np.int64) * 4 * C_EXACT   # a response table over [0, 2^30): four thresholds per grey level
DT_EXACT = 1_396_755_360                           # 6 * lcm(1 .. 20), below 2^31
T_EXACT = T0 + np.arange(4, dtype=np.int64) * DT_EXACT
C_FAR = (1 << 28) + 3                              # m <= 11 from any int32 reference level
REF_LEVELS = np.array([-(1 << 31), -(1 << 31) + 1, -(1 << 30) - 5, -1, 0, 1 << 30, (1 << 31) - 1], np.int64)
CARRY_FIRST = (1 << 32) - 3                        # frames 2^32 - 3 .. 2^32 + 2: the carry at frame 3 of the call
WALK_MAX = 1 << 20
SATURATED = 999_999                                # Hz: rate_q * delta >= 2^32 for every delta >= 2 us
ON_OFF = dict(seed=12345, rate_on_hz=40, rate_off_hz=15)


def _noise_ref(noise):
    if "rate_hz" in noise:
        return dict(seed=noise["seed"], rate_on=rate_q(noise["rate_hz"]), rate_off=rate_q(noise["rate_hz"]))
    return dict(seed=noise["seed"], rate_on=rate_q(noise.get("rate_on_hz", 0)), rate_off=rate_q(noise.get("rate_off_hz", 0)))


def _case(name, frames, times, c_on, c_off=None, lut=None, ref=None, timestamps="linear", refractory_us=None, noise=None,
          first_frame=None):
    """One case: the thresholds in table units (the device takes c / 256 grey levels, which is exact in a float)."""
    c_off = c_on if c_off is None else c_off
    dev = dict(threshold=c_on / 256, threshold_off=c_off / 256, timestamps=timestamps)
    res = dict(c_on=c_on, c_off=c_off, timestamps=timestamps)
    if lut is not None:
        dev["response"], res["lut"] = lut, lut
    if ref is not None:
        dev["ref"], res["ref"] = (ref, ref) if isinstance(ref, str) else (np.ascontiguousarray(ref, np.int32), ref)
    if refractory_us is not None:
        dev["refractory_us"] = res["refractory_us"] = refractory_us
    if noise is not None:
        dev["noise"] = noise
        res.update(_noise_ref(noise))
    if first_frame is not None:
        dev["first_frame"] = res["first_frame"] = first_frame
    return name, frames, np.asarray(times, np.int64), dev, res


@functools.lru_cache(maxsize=None)
def _random(seed, shape):
    f = np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def frames9():
    """The 9 x 19 x 37 stack of tests/test_events_sensor_gpu.py."""
    f = drifting_texture(9, 19, 37)
    f[4] = f[3]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def ref_plane():
    """D's reference plane: every one of REF_LEVELS many times over 19 x 37."""
    return REF_LEVELS[np.random.default_rng(41).integers(0, len(REF_LEVELS), (19, 37))]


def walk_frames():
    f = np.zeros((2, 3, 4), np.uint8)
    f[1, 1, 2] = 1
    return f


def walk_lut(step):
    lut = np.zeros(256, np.int64)
    lut[1] = step
    return lut


@functools.lru_cache(maxsize=None)
def top_frames():
    """4 x 5 x 7 random; pixel (0, 0) stays black and then rises by exactly one threshold of 10 grey levels at the last frame:
    its crossing is stamped times[n-1] in either mode."""
    f = np.random.default_rng(43).integers(0, 256, (4, 5, 7), dtype=np.uint8)
    f[:, 0, 0] = (0, 0, 0, 10)
    f.setflags(write=False)
    return f


TOP_REFRACTORY = 700
T_TOP_SENSOR = np.int64(INT64_MAX - TOP_REFRACTORY) - np.array([3000, 2000, 1000, 0], np.int64)   # times[n-1] + refractory_us = INT64_MAX
T_TOP = np.int64(INT64_MAX) - np.array([3000, 2000, 1000, 0], np.int64)


@functools.lru_cache(maxsize=None)
def _all():
    out = []
    for mode in MODES:
        out.append(_case(f"A-wide-{mode}", _random(31, (3, 1, 32767)), T_SHORT, 40 * 256, timestamps=mode))
        out.append(_case(f"A-tall-{mode}", _random(32, (3, 32767, 1)), T_SHORT, 40 * 256, timestamps=mode))
        out.append(_case(f"A-353wg-{mode}", _random(33, (3, 300, 301)), T_SHORT, 40 * 256, timestamps=mode))
        out.append(_case(f"A-wide-sensor-{mode}", _random(31, (3, 1, 32767)), T_SHORT, 40 * 256, timestamps=mode, refractory_us=11111,
                         noise=ON_OFF))
    out.append(_case("B-linear", _random(34, (4, 37, 53)), T_WIDE, 10 * 256))
    out.append(_case("C-plain-linear", _random(34, (4, 37, 53)), T_WIDE, C_STEEP, lut=STEEP))
    out.append(_case("C-sensor-linear", _random(34, (4, 37, 53)), T_WIDE, C_STEEP, lut=STEEP, refractory_us=1))
    out.append(_case("C-exact-plain-linear", _random(36, (4, 13, 17)), T_EXACT, C_EXACT, lut=EXACT, ref="first"))
    out.append(_case("C-exact-sensor-linear", _random(36, (4, 13, 17)), T_EXACT, C_EXACT, lut=EXACT, ref="first", refractory_us=1))
    for mode in MODES:
        out.append(_case(f"D-plain-{mode}", _random(35, (3, 19, 37)), T_SHORT, C_FAR, lut=STEEP, ref=ref_plane(), timestamps=mode))
        out.append(_case(f"D-sensor-{mode}", _random(35, (3, 19, 37)), T_SHORT, C_FAR, lut=STEEP, ref=ref_plane(), timestamps=mode,
                         refractory_us=700))
    for mode in MODES:
        for kind, noise in (("on/off", ON_OFF), ("saturated", dict(seed=12345, rate_hz=SATURATED))):
            out.append(_case(f"E-{kind}-{mode}", frames9()[:6], T_SENSOR, 10 * 256, 7 * 256, timestamps=mode, refractory_us=500,
                             noise=noise, first_frame=CARRY_FIRST))
    t_walk = [0, 1 << 21]
    out.append(_case("F-below-linear", walk_frames(), t_walk, 1, lut=walk_lut(WALK_MAX - 1), refractory_us=1))
    out.append(_case("F-at-frame", walk_frames(), t_walk, 1, lut=walk_lut(WALK_MAX), timestamps="frame", refractory_us=1))
    out.append(_case("F-at-linear-no-walk", walk_frames(), t_walk, 1, lut=walk_lut(WALK_MAX), refractory_us=0, first_frame=1))
    for mode in MODES:
        out.append(_case(f"G-sensor-{mode}", top_frames(), T_TOP_SENSOR, 10 * 256, timestamps=mode, refractory_us=TOP_REFRACTORY,
                         noise=ON_OFF))
        out.append(_case(f"G-plain-{mode}", top_frames(), T_TOP, 10 * 256, timestamps=mode))
    out.append(_case("G-noise-alone-linear", top_frames(), T_TOP, 10 * 256, noise=ON_OFF))
    return {c[0]: c for c in out}


def cases(group=None):
    """(name, frames, times, device keyword arguments, restatement keyword arguments) of every case, or of one group (a letter)."""
    for name, c in _all().items():
        if group is None or name.startswith(group + "-"):
            yield c


def names(group=None):
    return [c[0] for c in cases(group)]


def case(name):
    return _all()[name]


# F's refused call: the step of exactly 2^20 crossings under a linear walk (no restatement: there is no stream)
F_REFUSED = _case("F-at-linear", walk_frames(), [0, 1 << 21], 1, lut=walk_lut(WALK_MAX), refractory_us=1)


def is_sensor(res):
    return any(k in res for k in SENSOR_KEYS)


def restate(frames, times, res, **over):
    """The restatement of a case's call (over: arguments changed or added)."""
    kw = dict(res, **over)
    c_on, c_off = kw.pop("c_on"), kw.pop("c_off")
    return (events_sensor_ref if is_sensor(kw) else events_from_frames_ref)(frames, times, c_on, c_off, **kw)


@functools.lru_cache(maxsize=None)
def restatement(name):
    _, frames, times, _, res = case(name)
    out = restate(frames, times, res)
    for v in out.values():
        v.setflags(write=False)
    return out


def frozen_high_word(first_frame, k):
    """A wrong noise counter: the third word taken from first_frame, not from first_frame + k."""
    return ((first_frame >> 32) << 32) | ((first_frame + k) & 0xFFFFFFFF)


# ---- what makes each case a limit case, on the restatement alone ----------------------------------------------------------
def _pre_a(name):
    _, frames, _, _, _ = case(name)
    ev = restatement(name)
    n, h, w = frames.shape
    assert ev["x"].max() == w - 1 and ev["y"].max() == h - 1 and ev["x"].min() == 0 and ev["y"].min() == 0
    if "353wg" in name:
        n_wg = -(-h * w // 256)
        assert n_wg == 353 and w % 256 and 256 % w   # more than one 256-entry chunk of a table row; rows straddle workgroups
        pix = ev["y"].astype(np.int64) * w + ev["x"]
        assert (pix >= 256 * 256).any() and (pix >= 352 * 256).any()   # events of workgroups behind the first chunk, and of the last
    else:
        assert max(h, w) == 32767 and ("sensor" in name or 150_000 < len(ev["x"]) < 250_000)
    if "sensor" in name:   # noise drawn, events dropped
        assert ev["noise"].min() > 100 and 20_000 < len(ev["x"]) < len(restatement(name.replace("-sensor", ""))["x"]) + ev["noise"].sum()


def _pre_b(name):
    _, _, times, _, _ = case(name)
    t = restatement(name)["t"]
    assert int((t - times[0]).max()) >= 1 << 32 and t.min() < 0 and int(times[-1] - times[0]).bit_length() == 33
    assert (t > 0).any() and int(np.diff(times).max()) < 1 << 31


def stamp_terms(name):
    """(num, dt, den, t) of every linear stamp of the plain model on a case's input, as Python ints."""
    _, frames, times, _, res = case(name)
    terms = []
    plain = {k: v for k, v in res.items() if k not in SENSOR_KEYS}
    restate(frames, times, plain, on_stamps=lambda k, num, dt, den, t: terms.extend(zip(num.tolist(), [dt] * len(num), den.tolist(), t.tolist())))
    return terms


def _pre_c(name):
    """Products beyond 2^53 in every C case.  A stamp that a quotient formed in double gets wrong needs more: the error of the
    double quotient is below 2^-21, so it shows only where the true quotient is a whole number (or that close to one).  On
    the steep table with c = 3 * 2^22 + 1 and the wide times no quotient is: 163671 of the 164947 products exceed 2^53 and
    not one stamp differs.  The C-exact cases are built for it: from ref="first" every level is a whole multiple of the
    threshold, a step of g grey levels is 4 g thresholds, and the interval is a multiple of 1 .. 20, so the quotient
    j * dt / (4 g) is whole for most g and the 61-bit product is not a double: 3917 of the 215516 stamps differ."""
    terms = stamp_terms(name)
    big = [(num, dt, den, t) for num, dt, den, t in terms if num * dt > 1 << 53]
    # the quotient as a kernel would form it in double: two roundings, then the truncation
    off = [(num, dt, den, t) for num, dt, den, t in terms if int(float(num) * float(dt) / float(den)) != (num * dt) // den]
    assert len(big) > 1000 and max(num * dt for num, dt, _, _ in terms) < 1 << 61, len(big)
    if "exact" in name:
        assert len(off) > 1000, len(off)
    _, frames, _, _, res = case(name)
    m_max = int(np.abs(np.diff(res["lut"][frames].astype(np.int64), axis=0)).max()) // res["c_on"]
    assert m_max <= (1020 if "exact" in name else 85)   # far below the walk's limit
    if is_sensor(res):
        assert 1000 < len(restatement(name)["x"]) <= len(restatement(name.replace("sensor", "plain"))["x"])


def _pre_d(name):
    _, frames, _, _, res = case(name)
    ref = np.asarray(res["ref"], np.int64)
    assert sorted(np.unique(ref).tolist()) == sorted(REF_LEVELS.tolist()) and ref.min() == -(1 << 31) and ref.max() == (1 << 31) - 1
    d0 = np.abs(res["lut"][frames[0]] - ref)
    assert (d0 >= 1 << 31).sum() > 100 and d0.max() < 1 << 32 and d0.max() // res["c_on"] <= 11
    ev = restatement(name)
    assert ev["frame_bounds"][1] > 1000 or is_sensor(res)
    assert ev["ref"].dtype == np.int32 and len(ev["x"]) > 500


def _pre_e(name):
    _, frames, times, _, res = case(name)
    assert res["first_frame"] >> 32 == 0 and (res["first_frame"] + len(frames) - 1) >> 32 == 1
    ev, wrong = restatement(name), restate(frames, times, res, counter_of=frozen_high_word)
    same = all(np.array_equal(ev[k], wrong[k]) for k in ("x", "y", "p", "t", "frame_bounds", "t_ok"))
    if "saturated-frame" in name:
        # every pixel has both noise candidates in every interval and all are stamped T[k]: the stream does not depend on the
        # generator's words, so this one case of the four cannot see the counter
        assert same and (ev["noise"] == 19 * 37 * 5).all()
    else:
        assert not same
        cut = wrong["frame_bounds"][3]   # the frames before the carry are drawn alike
        assert np.array_equal(ev["frame_bounds"][:4], wrong["frame_bounds"][:4]) and np.array_equal(ev["t"][:cut], wrong["t"][:cut])


def _pre_f(name):
    _, frames, times, _, res = case(name)
    m = int(res["lut"][1]) // res["c_on"]
    ev = restatement(name)
    assert frames.sum() == 1 and res["c_on"] == 1 and ((ev["x"] == 2) & (ev["y"] == 1)).all()
    if name == "F-below-linear":
        assert m == WALK_MAX - 1 and len(ev["x"]) == m and np.diff(ev["t"]).min() >= 2   # every crossing survives the microsecond
    elif name == "F-at-frame":
        assert m == WALK_MAX and len(ev["x"]) == 1 and ev["t_ok"][1, 2] == times[1] + 1
    else:
        assert m == WALK_MAX and len(ev["x"]) == m and res["refractory_us"] == 0 and "t_ok" not in res and is_sensor(res)


def _pre_g(name):
    _, _, times, _, res = case(name)
    ev = restatement(name)
    assert int(ev["t"].max()) == int(times[-1]) and len(ev["x"]) > 50
    assert ((ev["x"] == 0) & (ev["y"] == 0) & (ev["t"] == times[-1])).sum() == 1   # the crossing stamped times[n-1] in either mode
    if res.get("refractory_us"):
        assert int(times[-1]) + res["refractory_us"] == INT64_MAX and ev["t_ok"][0, 0] == INT64_MAX
    else:
        assert int(times[-1]) == INT64_MAX
    if "seed" in res:
        assert ev["noise"].sum() > 0


PRECONDITIONS = {"A": _pre_a, "B": _pre_b, "C": _pre_c, "D": _pre_d, "E": _pre_e, "F": _pre_f, "G": _pre_g}


def precondition(name):
    PRECONDITIONS[name[0]](name)
