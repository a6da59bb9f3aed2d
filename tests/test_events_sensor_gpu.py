"""GPU: events_from_frames_dev with a refractory period and background-activity noise against the restatement of the sensor
model (tests/events_sensor_ref.py).  Everything is integer: x, y, p, t, frame_bounds, ref and t_ok must be equal, no
tolerance."""
import ctypes as C

import numpy as np
import pytest

from events_from_frames_ref import drifting_texture, events_from_frames_ref, log_lut, units
from events_sensor_ref import NEVER, events_sensor_ref, rate_q

pytestmark = pytest.mark.gpu

TIMES = np.array([5, 33338, 50005, 120005, 121005, 200005, 233338, 233345, 300005], np.int64)   # uneven; gaps 7 us .. 79 ms
THIRD, TWO = 11111, 70000                       # a third of a frame interval, two intervals
SATURATED = 999_999                             # Hz: rate_q * delta >= 2^32 for every delta >= 2 us
KEYS = ("x", "y", "p", "t", "frame_bounds", "ref", "t_ok")


def _hot(h, w):
    maps = np.zeros((h, w, 2))
    maps[h // 2, w // 3] = (5000.0, 20000.0)
    return maps


def _noise(kind, h, w, seed=12345):
    return {"none": None, "zero": dict(seed=seed, rate_hz=0), "1hz": dict(seed=seed, rate_hz=1),
            "on/off": dict(seed=seed, rate_on_hz=40, rate_off_hz=15), "saturated": dict(seed=seed, rate_hz=SATURATED),
            "hot": dict(seed=seed, rate_maps=_hot(h, w))}[kind]


def _dev(a, torch_dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch_dev)


def _host(res, ctx):
    ctx.synchronize()
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in res.items()}


def _assert_equal(got, want, what=""):
    assert got["x"].dtype == np.int16 and got["y"].dtype == np.int16 and got["p"].dtype == np.int8 and got["t"].dtype == np.int64
    assert got["frame_bounds"].dtype == np.int64 and got["ref"].dtype == np.int32 and got["t_ok"].dtype == np.int64
    assert np.array_equal(got["frame_bounds"], want["frame_bounds"]), (what, got["frame_bounds"], want["frame_bounds"])
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)


def _ref_kw(kw):
    """The restatement's arguments for the keyword arguments of a device call."""
    out = {k: kw[k] for k in ("timestamps", "p_on", "p_off", "refractory_us", "first_frame") if k in kw}
    noise = kw.get("noise")
    if noise is not None:
        out["seed"] = noise["seed"]
        if "rate_maps" in noise:
            q = np.rint(np.asarray(noise["rate_maps"], np.float64) * 4294967296.0 / 1e6).astype(np.uint64)
            out["rate_on"], out["rate_off"] = q[..., 0], q[..., 1]
        elif "rate_hz" in noise:
            out["rate_on"] = out["rate_off"] = rate_q(noise["rate_hz"])
        else:
            out["rate_on"], out["rate_off"] = rate_q(noise.get("rate_on_hz", 0)), rate_q(noise.get("rate_off_hz", 0))
    for k in ("ref", "t_ok"):
        v = kw.get(k)
        if v is not None:
            out[k] = v if isinstance(v, str) else v.cpu().numpy()
    if "response" in kw:
        out["lut"] = kw["response"]
    return out


def _run(nsof, ctx, torch_dev, frames, times, thr, thr_off=None, **kw):
    """The device run and the restatement of the same call (thresholds in grey levels)."""
    got = _host(nsof.events_from_frames_dev(_dev(frames, torch_dev), times, threshold=thr, threshold_off=thr_off, ctx=ctx, **kw), ctx)
    want = events_sensor_ref(frames, times, units(thr), units(thr if thr_off is None else thr_off), **_ref_kw(kw))
    return got, want


@pytest.fixture(scope="module")
def frames9():
    """9 x 19 x 37: 703 pixels, three workgroups, the last partial (its other threads walk pixel 0)."""
    f = drifting_texture(9, 19, 37)
    f[4] = f[3]   # an empty pair: noise alone
    return f


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
@pytest.mark.parametrize("n", [1, 4, 6, 9])
@pytest.mark.parametrize("shape", [(19, 37), (1, 1), (5, 3)])
def test_shapes_and_frame_counts(nsof_lib, ctx, torch_dev, shape, n, timestamps):
    """A partial last batch of frames, a partial last workgroup, a single pixel; refractory time and saturated noise at once."""
    h, w = shape
    frames = np.random.default_rng(h * 100 + n).integers(0, 256, (n, h, w), dtype=np.uint8)
    got, want = _run(nsof_lib, ctx, torch_dev, frames, TIMES[:n], 6.0, 9.0, timestamps=timestamps, refractory_us=THIRD,
                     noise=_noise("saturated", h, w), first_frame=3)
    assert (want["noise"] == h * w * (n - 1)).all() and (n == 1 or len(want["x"]) >= h * w)
    _assert_equal(got, want)


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
@pytest.mark.parametrize("ref", [None, "first"])
@pytest.mark.parametrize("refractory_us,noise", [(r, k) for r in (0, 1, THIRD, TWO) for k in ("none", "zero", "1hz", "on/off", "saturated", "hot")
                                                  if r or k != "none"])   # (0, none): the plain generator, tested below
def test_refractory_times_and_noise_rates(nsof_lib, ctx, torch_dev, frames9, refractory_us, noise, ref, timestamps):
    """Each refractory time alone and with each noise rate.  ref=None gives a dozen and more same-stamp crossings per pixel
    at frame 0, of which a refractory time keeps one."""
    frames, times = frames9[:6], TIMES[:6]
    got, want = _run(nsof_lib, ctx, torch_dev, frames, times, 10.0, 7.0, ref=ref, timestamps=timestamps, refractory_us=refractory_us,
                     noise=_noise(noise, 19, 37), first_frame=1 << 40)
    plain = events_from_frames_ref(frames, times, units(10), units(7), ref=ref, timestamps=timestamps)
    assert np.array_equal(want["ref"], plain["ref"])
    if noise in ("none", "zero"):
        assert not want["noise"].any() and len(want["x"]) <= len(plain["x"])
        assert (len(want["x"]) == len(plain["x"])) == (refractory_us == 0) or refractory_us == 1
    elif noise == "hot":
        assert want["noise"].min() >= 3
    else:
        assert want["noise"].min() > (20 if noise == "1hz" else 500)
    if ref is None and refractory_us:
        assert want["frame_bounds"][1] == 19 * 37 - (frames[0] < 10).sum()   # one event per pixel that crosses at all
    _assert_equal(got, want)


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_padded_strides_and_a_logarithmic_response(nsof_lib, ctx, torch_dev, frames9, timestamps):
    import torch
    big = torch.full((11, 23, 64), 200, dtype=torch.uint8, device=torch_dev)
    view = big[1:10, 2:21, 5:42]
    view.copy_(_dev(frames9, torch_dev))
    assert not view.is_contiguous()
    lut = log_lut()
    kw = dict(timestamps=timestamps, refractory_us=THIRD, noise=_noise("on/off", 19, 37), response=lut)
    got = _host(nsof_lib.events_from_frames_dev(view, TIMES, threshold=9.0, threshold_off=14.0, ctx=ctx, **kw), ctx)
    _assert_equal(got, events_sensor_ref(frames9, TIMES, units(9), units(14), **_ref_kw(kw)))


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_the_long_walk_at_the_finest_threshold(nsof_lib, ctx, torch_dev, timestamps):
    """1/256 grey level on 5 x 3 with a refractory time of 1 us: three pixels swing 0 -> 255 -> 0, 65280 crossings per step.
    The first step takes 20 ms, three crossings per microsecond, of which the walk keeps one; the second takes 180 ms."""
    frames = np.random.default_rng(3).integers(0, 256, (3, 5, 3), dtype=np.uint8)
    frames[:, 0, 0] = frames[:, 2, 1] = frames[:, 4, 2] = (0, 255, 0)
    times = np.array([0, 20_000, 200_000], np.int64)
    got, want = _run(nsof_lib, ctx, torch_dev, frames, times, 1 / 256, timestamps=timestamps, refractory_us=1,
                     noise=_noise("on/off", 5, 3))
    n_swing = int(((want["x"] == 0) & (want["y"] == 0)).sum())
    assert n_swing == 2 if timestamps == "frame" else 20_000 + 65280 <= n_swing <= 20_000 + 65280 + 4
    _assert_equal(got, want)


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
@pytest.mark.parametrize("refractory_us,noise", [(0, "on/off"), (THIRD, "on/off"), (TWO, "none"), (1, "saturated")])
def test_chunked_at_every_cut_equals_one_shot(nsof_lib, ctx, torch_dev, frames9, timestamps, refractory_us, noise):
    frames, times = frames9[:6], TIMES[:6]
    d = _dev(frames, torch_dev)
    kw = dict(threshold=5.0, threshold_off=8.0, ref="first", timestamps=timestamps, refractory_us=refractory_us,
              noise=_noise(noise, 19, 37), ctx=ctx)
    one = _host(nsof_lib.events_from_frames_dev(d, times, first_frame=100, **kw), ctx)
    _assert_equal(one, events_sensor_ref(frames, times, units(5), units(8), first_frame=100, **_ref_kw(kw)))
    for k in range(6):
        a = nsof_lib.events_from_frames_dev(d[:k + 1], times[:k + 1], first_frame=100, **kw)
        ctx.synchronize()
        b = _host(nsof_lib.events_from_frames_dev(d[k:], times[k:], first_frame=100 + k, t_ok=a["t_ok"], **dict(kw, ref=a["ref"])), ctx)
        a = _host(a, ctx)
        assert b["frame_bounds"][1] == 0
        for key in "xypt":
            assert np.array_equal(np.concatenate([a[key], b[key]]), one[key]), (k, key)
        assert np.array_equal(np.concatenate([a["frame_bounds"], a["frame_bounds"][-1] + b["frame_bounds"][2:]]), one["frame_bounds"])
        assert np.array_equal(b["ref"], one["ref"]) and np.array_equal(b["t_ok"], one["t_ok"])


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
@pytest.mark.parametrize("noise", ["none", "on/off"])
def test_a_given_t_ok_plane_without_a_refractory_time(nsof_lib, ctx, torch_dev, frames9, noise, timestamps):
    """Pixels blocked until times spread over the sequence (and some never blocked, some for ever); two runs, one result."""
    rng = np.random.default_rng(8)
    t_ok = rng.integers(0, 260_000, (19, 37)).astype(np.int64)
    t_ok[rng.random((19, 37)) < 0.2] = NEVER
    t_ok[0, :5] = np.iinfo(np.int64).max
    kw = dict(timestamps=timestamps, noise=_noise(noise, 19, 37), t_ok=_dev(t_ok, torch_dev))
    got, want = _run(nsof_lib, ctx, torch_dev, frames9, TIMES, 10.0, **kw)
    plain = events_from_frames_ref(frames9, TIMES, units(10), units(10), timestamps=timestamps)
    assert len(want["x"]) > 1000 and (noise != "none" or len(want["x"]) < len(plain["x"]))
    assert not ((want["y"] == 0) & (want["x"] < 5)).any()
    _assert_equal(got, want)
    again, _ = _run(nsof_lib, ctx, torch_dev, frames9, TIMES, 10.0, **kw)
    _assert_equal(again, got)


def test_default_arguments_take_the_plain_entries(nsof_lib, ctx, torch_dev, frames9):
    d = _dev(frames9, torch_dev)
    plain = _host(nsof_lib.events_from_frames_dev(d, TIMES, threshold=10.0, ctx=ctx), ctx)
    same = _host(nsof_lib.events_from_frames_dev(d, TIMES, threshold=10.0, refractory_us=0, noise=None, t_ok=None, first_frame=0, ctx=ctx), ctx)
    assert sorted(plain) == sorted(same) == ["frame_bounds", "p", "ref", "t", "x", "y"]
    want = events_from_frames_ref(frames9, TIMES, units(10), units(10))
    for k in plain:
        assert np.array_equal(plain[k], want[k]) and np.array_equal(same[k], want[k]), k
    # the sensor entries with nothing to do give the same stream, and t_ok besides
    quiet = _host(nsof_lib.events_from_frames_dev(d, TIMES, threshold=10.0, noise=dict(seed=5, rate_hz=0), ctx=ctx), ctx)
    assert sorted(quiet) == sorted(KEYS)
    for k in plain:
        assert np.array_equal(quiet[k], want[k]), k
    assert np.array_equal(quiet["t_ok"], events_sensor_ref(frames9, TIMES, units(10), units(10))["t_ok"])


def test_video_to_flow_sequence_forwards_the_sensor_arguments(nsof_lib, ctx, torch_dev):
    from nsof import pipeline
    frames = drifting_texture(8, 64, 96)
    sensor = dict(refractory_us=800, noise=dict(seed=21, rate_hz=30), first_frame=7)
    acc = dict(slice_us=1000, snapshot_every=5, refractory_us=500)   # the accumulator's own refractory time
    d = _dev(frames, torch_dev)
    surfaces, flows, ev = pipeline.video_to_flow_sequence(d, frame_us=5000, threshold=10.0, p_off=0, sensor=sensor, ctx=ctx, **acc)
    direct = _host(nsof_lib.events_from_frames_dev(d, frame_us=5000, threshold=10.0, p_off=0, ctx=ctx, **sensor), ctx)
    ev = _host(ev, ctx)
    _assert_equal(ev, direct)
    _assert_equal(direct, events_sensor_ref(frames, np.arange(8, dtype=np.int64) * 5000, units(10), units(10), p_off=0,
                                            **_ref_kw(sensor)))
    assert surfaces.shape[0] == flows.shape[0] + 1 >= 2 and len(ev["x"]) > 10_000


def _struct(nsof_lib, **over):
    from nsof import _lib
    f = dict(refractory_us=800, seed=1, first_frame=0, rate_on_q=4295, rate_off_q=4295, d_rate_plane=None, d_t_ok_in=None)
    f.update(over)
    return _lib.EventsSensor(*(f[name] for name, _ in _lib.EventsSensor._fields_))


# what is wrong, the entry, the sensor struct's fields changed, other arguments changed, the status, what nsof_last_error names
C_REFUSALS = [
    ("refractory negative", "both", dict(refractory_us=-1), {}, "EINVAL", "refractory_us = -1 is outside [0, 2^31)"),
    ("refractory 2^31", "both", dict(refractory_us=1 << 31), {}, "EINVAL", "refractory_us = 2147483648 is outside"),
    ("first_frame negative", "both", dict(first_frame=-1), {}, "EINVAL", "first_frame = -1 with 6 frames"),
    ("first_frame beyond 2^62", "both", dict(first_frame=(1 << 62) - 5), {}, "EINVAL", "first_frame = 4611686018427387899 with 6 frames"),
    ("timestamps_mode unknown", "both", {}, dict(mode=2), "EINVAL", "timestamps_mode 2"),
    ("t_ok_in without t_ok_out", "emit", dict(d_t_ok_in="plane"), dict(t_ok_out=None), "EINVAL", "d_t_ok_in without d_t_ok_out"),
    ("c_on 0 (the shared check)", "both", {}, dict(c_on=0), "EINVAL", "thresholds c_on = 0, c_off = 1792"),
    ("t_ok beyond int64", "both", {}, dict(times=np.iinfo(np.int64).max - 799 + 1000 * np.arange(-5, 1, dtype=np.int64)), "EINVAL",
     "times[5] = 9223372036854775008 with refractory_us = 800"),
]


@pytest.fixture(scope="module")
def c_stack(nsof_lib, ctx, torch_dev, frames9):
    """The 6 x 19 x 37 stack on the device, the bounds of a good call of the sensor count entry, and marked outputs."""
    import torch
    from nsof import _lib
    d = _dev(frames9[:6], torch_dev)
    times, lut = TIMES[:6].copy(), np.arange(256, dtype=np.int32) * 256
    bounds = np.full(7, -1, np.int64)
    st = _struct(nsof_lib)
    torch.cuda.synchronize()
    rc = ctx._lib.nsof_events_from_frames_sensor_count_dev(ctx.ptr, d.data_ptr(), d.stride(1), d.stride(0), 6, 19, 37, times.ctypes.data,
                                                           lut.ctypes.data, 2560, 1792, None, None, 0, 1, C.byref(st), bounds.ctypes.data)
    assert rc == _lib.NSOF_OK and bounds[-1] > 1000
    total = int(bounds[-1])
    out = dict(x=torch.full((total,), -7, dtype=torch.int16, device=torch_dev), y=torch.full((total,), -7, dtype=torch.int16, device=torch_dev),
               p=torch.full((total,), -7, dtype=torch.int8, device=torch_dev), t=torch.full((total,), -7, dtype=torch.int64, device=torch_dev),
               ref=torch.full((19, 37), -7, dtype=torch.int32, device=torch_dev),
               t_ok=torch.full((19, 37), -7, dtype=torch.int64, device=torch_dev))
    torch.cuda.synchronize()
    return d, times, lut, bounds, out


@pytest.mark.parametrize("what,entries,fields,over,status,message", C_REFUSALS, ids=[r[0] for r in C_REFUSALS])
def test_c_entries_refuse_before_any_launch(nsof_lib, ctx, c_stack, what, entries, fields, over, status, message):
    from nsof import _lib
    d, times, lut, bounds, out = c_stack
    fields = dict(fields)
    if fields.get("d_t_ok_in") == "plane":
        fields["d_t_ok_in"] = out["t_ok"].data_ptr()
    st = _struct(nsof_lib, **fields)
    a = dict(mode=1, c_on=2560, t_ok_out=out["t_ok"].data_ptr(), times=times)
    a.update(over)
    common = (ctx.ptr, d.data_ptr(), d.stride(1), d.stride(0), 6, 19, 37, a["times"].ctypes.data, lut.ctypes.data, a["c_on"], 1792, None, None, 0)
    for entry in ("count", "emit") if entries == "both" else (entries,):
        if entry == "count":
            b = np.full(7, -1, np.int64)
            rc = ctx._lib.nsof_events_from_frames_sensor_count_dev(*common, a["mode"], C.byref(st), b.ctypes.data)
            assert (b == -1).all()
        else:
            rc = ctx._lib.nsof_events_from_frames_sensor_emit_dev(*common, bounds.ctypes.data, a["mode"], 1, -1, int(bounds[-1]),
                                                                  out["x"].data_ptr(), out["y"].data_ptr(), out["p"].data_ptr(),
                                                                  out["t"].data_ptr(), out["ref"].data_ptr(), C.byref(st), a["t_ok_out"])
        msg = ctx._lib.nsof_last_error(ctx.ptr).decode()
        assert rc == getattr(_lib, "NSOF_" + status) and message in msg and f"sensor_{entry}" in msg, (entry, rc, msg)
        ctx.synchronize()
        assert all(bool((v == -7).all()) for v in out.values())


def test_c_entries_with_a_null_struct_and_with_bounds_of_another_mode(nsof_lib, ctx, c_stack, frames9):
    """sensor == NULL: the plain pair's result, t_ok_out untouched.  The counts depend on the stamp mode under a refractory
    time: bounds counted for linear stamps do not fit the frame-stamped run, and the emit pass writes nothing."""
    from nsof import _lib
    d, times, lut, bounds, out = c_stack
    common = (ctx.ptr, d.data_ptr(), d.stride(1), d.stride(0), 6, 19, 37, times.ctypes.data, lut.ctypes.data, 2560, 1792, None, None, 0)
    ptrs = tuple(out[k].data_ptr() for k in ("x", "y", "p", "t", "ref"))
    st = _struct(nsof_lib)
    b_frame = np.full(7, -1, np.int64)
    assert ctx._lib.nsof_events_from_frames_sensor_count_dev(*common, 0, C.byref(st), b_frame.ctypes.data) == _lib.NSOF_OK
    assert b_frame[-1] < bounds[-1]
    assert ctx._lib.nsof_events_from_frames_sensor_emit_dev(*common, bounds.ctypes.data, 0, 1, -1, int(bounds[-1]), *ptrs, C.byref(st),
                                                            out["t_ok"].data_ptr()) == _lib.NSOF_OK
    ctx.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())
    b_plain = np.full(7, -1, np.int64)
    assert ctx._lib.nsof_events_from_frames_sensor_count_dev(*common, 1, None, b_plain.ctypes.data) == _lib.NSOF_OK
    want = events_from_frames_ref(frames9[:6], times, 2560, 1792)
    assert np.array_equal(b_plain, want["frame_bounds"]) and b_plain[-1] > bounds[-1]


def test_a_step_of_2_to_the_20_crossings_is_refused_under_a_linear_walk(nsof_lib, ctx, torch_dev):
    """A table that spans [0, 2^30] at a threshold of one unit: grey 0 -> 1 is 2^22 crossings.  With linear stamps and a
    refractory time they would be walked one by one, which the count pass refuses; with frame stamps one survives."""
    from nsof import _lib
    from nsof.errors import NsofValueError
    lut = np.arange(256, dtype=np.int64) << 22
    frames = np.zeros((2, 3, 4), np.uint8)
    frames[1, 1, 2] = 1
    d = _dev(frames, torch_dev)
    kw = dict(frame_us=1000, threshold=1 / 256, response=lut, refractory_us=1, ctx=ctx)
    with pytest.raises(NsofValueError, match=r"crosses 2\^20 thresholds or more in one step") as e:
        nsof_lib.events_from_frames_dev(d, timestamps="linear", **kw)
    assert e.value.status == _lib.NSOF_EUNSUPPORTED
    got = _host(nsof_lib.events_from_frames_dev(d, timestamps="frame", **kw), ctx)
    assert got["x"].tolist() == [2] and got["y"].tolist() == [1] and got["t"].tolist() == [1000] and got["ref"][1, 2] == 1 << 22
    assert got["t_ok"][1, 2] == 1001 and (got["t_ok"] == NEVER).sum() == 11
