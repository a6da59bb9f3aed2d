"""CPU: the limit cases of the event generator (tests/events_limits_cases.py) without a device.  Each case's preconditions are
asserted on the restatement; the restatements themselves (NumPy int64) are checked on these inputs against a scalar walk of the
model in plain Python integers, one pixel at a time, which cannot overflow: the reference holds where the kernels are meant to
be tested.  And the Python layer's refusal of a t_ok beyond the int64 range."""
import numpy as np
import pytest

import events_limits_cases as L  # noqa: N812
from accum_c2c_ref import M0, M1, W0, W1
from events_sensor_ref import NOISE_WORD

MASK = 0xFFFFFFFF
NEVER = -(1 << 63)
_M0, _M1, _W0, _W1 = int(M0), int(M1), int(W0), int(W1)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on Python ints."""
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + _W0) & MASK, (k1 + _W1) & MASK
    return c0, c1, c2, c3


def test_the_scalar_philox_gives_the_known_answer():
    assert philox(0, 0, 0, 0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


def walk_pixel(pix, grey, times, lut, c_on, c_off, r, timestamps, sensor, refractory_us=0, seed=0, rate_on=0, rate_off=0, t_ok=NEVER,
               first_frame=0):
    """The model of include/nsof.h for one pixel, every quantity a Python int -> (per frame the list of (t, polarity 0 / 1, j)
    in stream order, the final r, the final t_ok).  sensor False: the plain model, no walk."""
    out, prev = [], None
    for k, g in enumerate(grey):
        b, d = lut[g], lut[g] - r
        m, pol, c, sign = (d // c_on, 0, c_on, 1) if d >= c_on else ((-d) // c_off, 1, c_off, -1) if -d >= c_off else (0, 0, c_on, 1)
        same = timestamps == "frame" or k == 0
        cands = []   # (t, kind, j, polarity)
        for j in range(1, m + 1):
            if same:
                t = times[k]
            else:
                num, den = abs(r + sign * j * c - prev), abs(b - prev)
                assert 0 < num <= den
                t = times[k - 1] + (num * (times[k] - times[k - 1])) // den
            cands.append((t, 0, j, pol))
        r += sign * m * c
        assert -c_off < b - r < c_on and -(1 << 31) <= r < 1 << 31
        if sensor and k >= 1 and (rate_on or rate_off):
            f, delta = first_frame + k, times[k] - times[k - 1]
            w = philox(pix, f & MASK, f >> 32, NOISE_WORD, seed & MASK, seed >> 32)
            for npol, rate, draw, place in ((0, rate_on, w[0], w[2]), (1, rate_off, w[1], w[3])):
                if draw < min(MASK, rate * delta):
                    cands.append((times[k] if same else times[k - 1] + ((place * delta) >> 32), 1 + npol, (m if npol == pol else 0) + 1, npol))
        kept = []
        for t, kind, j, p in sorted(cands):   # (t, signal before ON noise before OFF noise, crossing)
            if not sensor or t >= t_ok:
                kept.append((t, p, j))
                if sensor:
                    t_ok = t + refractory_us
        assert -(1 << 63) <= t_ok < 1 << 63
        out.append(sorted(kept))
        prev = b
    return out, r, t_ok


def check_pixels(name, pixels):
    _, frames, times, _, res = L.case(name)
    ev = L.restatement(name)
    n, h, w = frames.shape
    sensor = L.is_sensor(res)
    lut = [int(v) for v in (res["lut"] if "lut" in res else np.arange(256) * 256)]
    tl = [int(v) for v in times]
    ref = res.get("ref")
    kw = {k: int(res[k]) for k in ("refractory_us", "seed", "rate_on", "rate_off", "first_frame") if k in res}
    fb = ev["frame_bounds"].tolist()
    evx, evy, evt, evp = ev["x"].astype(np.int64), ev["y"].astype(np.int64), ev["t"], ev["p"]
    for pix in pixels:
        y, x = divmod(int(pix), w)
        grey = [int(v) for v in frames[:, y, x]]
        r0 = 0 if ref is None else lut[grey[0]] if isinstance(ref, str) else int(ref[y, x])
        per_frame, r, t_ok = walk_pixel(int(pix), grey, tl, lut, int(res["c_on"]), int(res["c_off"]), r0, res["timestamps"], sensor, **kw)
        mine = np.flatnonzero((evx == x) & (evy == y))
        for k in range(n):
            sel = mine[(mine >= fb[k]) & (mine < fb[k + 1])]
            got = [(int(t), 0 if p == 1 else 1) for t, p in zip(evt[sel].tolist(), evp[sel].tolist())]
            assert got == [(t, p) for t, p, _ in per_frame[k]], (name, pix, k)
        assert int(ev["ref"][y, x]) == r, (name, pix)
        if sensor:
            assert int(ev["t_ok"][y, x]) == t_ok, (name, pix)


def _crop(name):
    """Every pixel of the small cases; of the large ones both ends and two stretches inside."""
    _, frames, _, _, _ = L.case(name)
    npx = frames.shape[1] * frames.shape[2]
    if name[0] in "DEG":
        return range(npx)
    if name[0] == "A":
        return sorted({*range(40), *range(npx - 40, npx), *range(npx // 2, npx // 2 + 40), *range(65500, min(65580, npx))})
    return range(0, npx, 13)   # B, C: 151 of the 1961 pixels


@pytest.mark.parametrize("name", L.names())
def test_preconditions_hold_on_the_restatement(name):
    L.precondition(name)
    ev = L.restatement(name)
    assert (np.diff(ev["t"]) >= 0).all() and ev["frame_bounds"][-1] == len(ev["x"]) == len(ev["y"]) == len(ev["p"]) == len(ev["t"])


@pytest.mark.parametrize("name", [n for n in L.names() if n[0] != "F"])
def test_the_restatement_equals_a_scalar_walk_in_python_integers(name):
    check_pixels(name, _crop(name))


def test_the_walks_limit_case_is_one_pixel_of_known_stamps():
    """F: 2^20 - 1 crossings of one unit over 2^21 us are stamped (j * 2^21) // (2^20 - 1), each at least 2 us after the last."""
    ev = L.restatement("F-below-linear")
    m = L.WALK_MAX - 1
    assert ev["t"].tolist() == [(j << 21) // m for j in range(1, m + 1)] and ev["ref"][1, 2] == m and ev["t_ok"][1, 2] == (1 << 21) + 1
    ev = L.restatement("F-at-linear-no-walk")
    assert ev["t"].tolist() == [2 * j for j in range(1, L.WALK_MAX + 1)] and ev["t_ok"][1, 2] == 1 << 21


def test_every_group_has_its_cases():
    assert sorted({n[0] for n in L.names()}) == list("ABCDEFG") and len(L.names()) == len(set(L.names())) == 29
    for name, frames, times, dev, res in L.cases():
        assert frames.dtype == np.uint8 and times.dtype == np.int64 and len(times) == len(frames)
        assert round(dev["threshold"] * 256) == res["c_on"] and round(dev["threshold_off"] * 256) == res["c_off"]


def _cpu_frames():
    import torch
    return torch.zeros((4, 5, 7), dtype=torch.uint8)


def test_python_layer_refuses_a_t_ok_beyond_int64_before_any_device_work(nsof_lib):
    """The stack is a CPU tensor: a call that got past the check raises the 'must be CUDA tensors' error instead."""
    from nsof import _lib
    from nsof.errors import NsofValueError
    top = L.T_TOP_SENSOR
    for mode in L.MODES:
        with pytest.raises(NsofValueError, match=rf"times_us\[3\] = {int(top[-1]) + 1} with refractory_us = 700: t_ok = t \+ refractory_us") as e:
            nsof_lib.events_from_frames_dev(_cpu_frames(), top + 1, refractory_us=L.TOP_REFRACTORY, timestamps=mode)
        assert e.value.status == _lib.NSOF_EINVAL
    with pytest.raises(NsofValueError, match=r"times_us\[3\] = 9223372036854775807 with refractory_us = 1:"):
        nsof_lib.events_from_frames_dev(_cpu_frames(), L.T_TOP, refractory_us=1, noise=L.ON_OFF)
    # the largest times each call takes: up to INT64_MAX - refractory_us, and any int64 without a refractory time
    for times, kw in ((top, dict(refractory_us=L.TOP_REFRACTORY)), (L.T_TOP, {}), (L.T_TOP, dict(noise=L.ON_OFF)),
                      (L.T_TOP, dict(first_frame=5)), (L.T_TOP - 1, dict(refractory_us=1))):
        with pytest.raises(NsofValueError, match=r"frames \(and ref\) must be CUDA tensors on one device"):
            nsof_lib.events_from_frames_dev(_cpu_frames(), times, **kw)


def test_the_restatement_refuses_what_the_entries_refuse():
    _, frames, times, _, res = L.case("G-sensor-linear")
    with pytest.raises(AssertionError, match="t_ok would pass the int64 range"):
        L.restate(frames, times + 1, res)
