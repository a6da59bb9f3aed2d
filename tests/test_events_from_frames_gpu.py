"""GPU: events_from_frames_dev against the NumPy restatement of its model (tests/events_from_frames_ref.py).  Everything
is integer: x, y, p, t, frame_bounds and ref must be equal, no tolerance."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden_path
from events_from_frames_ref import drifting_texture, events_from_frames_ref, log_lut, units

pytestmark = pytest.mark.gpu

UNEVEN = np.array([0, 1000, 1700, 2100, 5000], np.int64)


def _dev(a, torch_dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch_dev)


def _host(res, ctx):
    ctx.synchronize()
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in res.items()}


def _assert_equal(got, want, what=""):
    assert got["x"].dtype == np.int16 and got["y"].dtype == np.int16 and got["p"].dtype == np.int8 and got["t"].dtype == np.int64
    assert got["frame_bounds"].dtype == np.int64 and got["ref"].dtype == np.int32
    assert np.array_equal(got["frame_bounds"], want["frame_bounds"]), (what, got["frame_bounds"], want["frame_bounds"])
    for k in ("x", "y", "p", "t", "ref"):
        assert np.array_equal(got[k], want[k]), (what, k)


def _run(nsof, ctx, torch_dev, frames, times, thr, thr_off=None, **kw):
    """The device run and the restatement of the same call (thresholds in grey levels)."""
    got = _host(nsof.events_from_frames_dev(_dev(frames, torch_dev), times, threshold=thr, threshold_off=thr_off, ctx=ctx, **kw), ctx)
    ref_kw = {k: kw[k] for k in ("timestamps", "p_on", "p_off") if k in kw}
    ref = kw.get("ref")
    want = events_from_frames_ref(frames, times, units(thr), units(thr if thr_off is None else thr_off), lut=kw.get("response"),
                                  ref=ref if ref is None or isinstance(ref, str) else ref.cpu().numpy(), **ref_kw)
    return got, want


@pytest.fixture(scope="module")
def random_frames():
    """5 x 37 x 53: 8 workgroups of 256 pixels, the last partial, rows straddling workgroups."""
    return np.random.default_rng(5).integers(0, 256, (5, 37, 53), dtype=np.uint8)


def test_small_box_sequence_gives_the_golden_events(nsof_lib, ctx, torch_dev):
    g = np.load(golden_path("synth_events.npz"))
    frames, times = nsof_lib.render_box_frames(H=60, W=90, box_h=20, box_w=11, speed_pps=700, duration_s=0.2)
    assert frames.shape == (400, 60, 90)
    got, want = _run(nsof_lib, ctx, torch_dev, frames, times, 1.0, timestamps="frame")
    assert len(got["x"]) == 3600
    for k in "xypt":
        assert np.array_equal(got[k], g[f"small_{k}"]), k
    _assert_equal(got, want)


@pytest.mark.parametrize("p_off", [0, -1])
@pytest.mark.parametrize("thr", [(10, 10), (7, 20), (300 / 256, 5000 / 256)])
@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_random_frames(nsof_lib, ctx, torch_dev, random_frames, timestamps, thr, p_off):
    got, want = _run(nsof_lib, ctx, torch_dev, random_frames, UNEVEN, thr[0], thr[1], timestamps=timestamps, p_off=p_off)
    assert len(want["x"]) > 1000 and set(np.unique(want["p"])) == {1, p_off}
    _assert_equal(got, want)


@pytest.mark.parametrize("shape", [(3, 256, 256), (3, 257, 256), (128, 13, 17), (129, 13, 17)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_scan_chunk_boundaries(nsof_lib, ctx, torch_dev, timestamps, shape):
    """The table scan at its chunk boundaries of 256 entries: 256 workgroups (a row of the table is exactly one chunk) and 257
    (a second chunk of one entry); 128 and 129 frames (256 row sums: one chunk; 258: a second chunk of two)."""
    frames = np.random.default_rng(31).integers(0, 256, shape, dtype=np.uint8)
    got, want = _run(nsof_lib, ctx, torch_dev, frames, np.arange(shape[0], dtype=np.int64) * 1000, 40, timestamps=timestamps)
    assert 10_000 < len(want["x"]) < 2_000_000
    _assert_equal(got, want)


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_full_swing_at_the_finest_threshold(nsof_lib, ctx, torch_dev, timestamps):
    """0 -> 255 -> 0 at 1/256 grey level: 65280 events per pixel and step -- the per-pixel emit loop, offsets far beyond
    a workgroup."""
    frames = np.zeros((3, 2, 3), np.uint8)
    frames[1] = 255
    got, want = _run(nsof_lib, ctx, torch_dev, frames, np.array([0, 70_000, 200_000], np.int64), 1 / 256, timestamps=timestamps)
    assert np.array_equal(want["frame_bounds"], [0, 0, 6 * 65280, 12 * 65280])
    _assert_equal(got, want)


def test_empty_pair_and_empty_stream(nsof_lib, ctx, torch_dev, random_frames):
    frames = random_frames.copy()
    frames[2] = frames[1]
    got, want = _run(nsof_lib, ctx, torch_dev, frames, UNEVEN, 4.0)
    assert want["frame_bounds"][2] == want["frame_bounds"][3] > 0
    _assert_equal(got, want)
    frames[:] = frames[0]
    got, want = _run(nsof_lib, ctx, torch_dev, frames, UNEVEN, 4.0, ref="first")
    assert not want["frame_bounds"].any() and got["x"].size == 0
    _assert_equal(got, want)


@pytest.mark.parametrize("ref", [None, "first"])
def test_single_frame(nsof_lib, ctx, torch_dev, random_frames, ref):
    got, want = _run(nsof_lib, ctx, torch_dev, random_frames[3:4], np.array([777], np.int64), 10.0, ref=ref)
    assert (len(want["x"]) == 0) == (ref == "first") and (want["t"] == 777).all()
    _assert_equal(got, want)


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_padded_strides(nsof_lib, ctx, torch_dev, random_frames, timestamps):
    import torch
    big = torch.full((7, 40, 64), 200, dtype=torch.uint8, device=torch_dev)
    view = big[1:6, 2:39, 5:58]
    view.copy_(_dev(random_frames, torch_dev))
    assert not view.is_contiguous()
    got = _host(nsof_lib.events_from_frames_dev(view, UNEVEN, threshold=6.0, timestamps=timestamps, ctx=ctx), ctx)
    _assert_equal(got, events_from_frames_ref(random_frames, UNEVEN, units(6), units(6), timestamps=timestamps))


def test_threshold_plane(nsof_lib, ctx, torch_dev, random_frames):
    plane = np.random.default_rng(2).integers(200, 9000, (37, 53, 2))   # table units, different per pixel and polarity
    got = _host(nsof_lib.events_from_frames_dev(_dev(random_frames, torch_dev), UNEVEN, threshold_maps=plane / 256.0, ctx=ctx), ctx)
    _assert_equal(got, events_from_frames_ref(random_frames, UNEVEN, plane[..., 0], plane[..., 1]))


def test_logarithmic_response(nsof_lib, ctx, torch_dev, random_frames):
    lut = log_lut()
    assert np.array_equal(lut, nsof_lib.log_response()) and (np.diff(lut) > 0).all() and lut[255] == 65280
    got, want = _run(nsof_lib, ctx, torch_dev, random_frames, UNEVEN, 9.0, 14.0, response=lut)
    _assert_equal(got, want)


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_chunked_at_every_cut_equals_one_shot(nsof_lib, ctx, torch_dev, timestamps):
    frames = np.random.default_rng(9).integers(0, 256, (6, 19, 31), dtype=np.uint8)
    times = np.array([10, 40, 45, 1000, 1001, 90_000], np.int64)
    d = _dev(frames, torch_dev)
    one = _host(nsof_lib.events_from_frames_dev(d, times, threshold=5.0, threshold_off=8.0, timestamps=timestamps, ctx=ctx), ctx)
    _assert_equal(one, events_from_frames_ref(frames, times, units(5), units(8), timestamps=timestamps))
    for k in range(6):
        a = nsof_lib.events_from_frames_dev(d[:k + 1], times[:k + 1], threshold=5.0, threshold_off=8.0, timestamps=timestamps, ctx=ctx)
        ctx.synchronize()
        b = _host(nsof_lib.events_from_frames_dev(d[k:], times[k:], threshold=5.0, threshold_off=8.0, ref=a["ref"],
                                                  timestamps=timestamps, ctx=ctx), ctx)
        a = _host(a, ctx)
        assert b["frame_bounds"][1] == 0
        for key in "xypt":
            assert np.array_equal(np.concatenate([a[key], b[key]]), one[key]), (k, key)
        assert np.array_equal(np.concatenate([a["frame_bounds"], a["frame_bounds"][-1] + b["frame_bounds"][2:]]), one["frame_bounds"])
        assert np.array_equal(b["ref"], one["ref"])


def test_linear_ties_keep_the_order_and_runs_repeat(nsof_lib, ctx, torch_dev, random_frames):
    """Frames 4 us apart: many pixels cross in the same microsecond, which pins (t, polarity, y, x, j) and the stability
    of the reorder; a second run gives the same bits."""
    times = np.arange(5, dtype=np.int64) * 4 + 100
    got, want = _run(nsof_lib, ctx, torch_dev, random_frames, times, 3.0, timestamps="linear")
    fb = want["frame_bounds"]
    assert max(np.unique(want["t"][fb[1]:fb[2]], return_counts=True)[1]) > 100
    _assert_equal(got, want)
    again = _host(nsof_lib.events_from_frames_dev(_dev(random_frames, torch_dev), times, threshold=3.0, timestamps="linear", ctx=ctx), ctx)
    _assert_equal(again, got)


def _count(nsof_lib, ctx, d_frames, times, c_on, c_off, d_plane=None, lut=None):
    """nsof_events_from_frames_count_dev itself -> (status, frame_bounds)."""
    import torch
    n, h, w = d_frames.shape
    times = np.ascontiguousarray(times, np.int64)
    lut = nsof_lib.linear_response() if lut is None else np.ascontiguousarray(lut, np.int32)
    bounds = np.full(n + 1, -1, np.int64)
    torch.cuda.synchronize()
    rc = ctx._lib.nsof_events_from_frames_count_dev(ctx.ptr, d_frames.data_ptr(), d_frames.stride(1), d_frames.stride(0), n, h, w,
                                                    times.ctypes.data, lut.ctypes.data, c_on, c_off,
                                                    None if d_plane is None else d_plane.data_ptr(), None, 0, bounds.ctypes.data)
    return rc, bounds


def test_two_to_the_31_events_are_refused_by_the_count(nsof_lib, ctx, torch_dev):
    """2^15 pixels swinging 0 -> 255 -> 0 at 1/256 grey level: one step is just under 2^31 events, two are over.  The emit
    pass never runs."""
    import torch
    from nsof import _lib
    from nsof.errors import NsofValueError
    frames = torch.zeros((3, 128, 256), dtype=torch.uint8, device=torch_dev)
    frames[1] = 255
    rc, bounds = _count(nsof_lib, ctx, frames[:2], [0, 10], 1, 1)
    assert rc == _lib.NSOF_OK and list(bounds) == [0, 0, 32768 * 65280] and bounds[2] < 1 << 31
    rc, bounds = _count(nsof_lib, ctx, frames, [0, 10, 20], 1, 1)
    assert rc == _lib.NSOF_EUNSUPPORTED and (bounds == -1).all()
    with pytest.raises(NsofValueError) as e:
        nsof_lib.events_from_frames_dev(frames, frame_us=10, threshold=1 / 256, ctx=ctx)
    assert e.value.status == _lib.NSOF_EUNSUPPORTED


def test_counts_of_2_to_the_24_and_more_per_pixel(nsof_lib, ctx, torch_dev):
    """A table that spans the whole [0, 2^30] at a threshold of one unit: single pixels emit 2^24 events and more per step,
    where the count pass leaves its 32-bit sums (count only: the stream would be a gigabyte)."""
    import torch
    from nsof import _lib
    lut = np.arange(256, dtype=np.int64) << 22
    frames = torch.zeros((3, 5, 67), dtype=torch.uint8, device=torch_dev)   # 335 pixels: two workgroups, the second partial
    grey = np.zeros((3, 5, 67), np.int64)
    grey[0, 0, :3] = (1, 3, 4)
    grey[1, 0, :3] = (9, 3, 0)
    grey[1, 4, 66] = 100
    grey[2, 4, 66] = 60
    frames.copy_(_dev(grey.astype(np.uint8), torch_dev))
    rc, bounds = _count(nsof_lib, ctx, frames, [0, 5, 9], 1, 1, lut=lut)
    per_frame = [(1 + 3 + 4) << 22, (8 + 4 + 100) << 22, (9 + 3 + 40) << 22]   # frame 2 is black but for one pixel
    assert rc == _lib.NSOF_OK and list(bounds) == list(np.concatenate([[0], np.cumsum(per_frame)]))


def test_small_capacity_and_zero_threshold_are_refused(nsof_lib, ctx, torch_dev, random_frames):
    import torch
    from nsof import _lib
    from nsof.errors import NsofValueError
    d = _dev(random_frames, torch_dev)
    rc, bounds = _count(nsof_lib, ctx, d, UNEVEN, 2560, 2560)
    total = int(bounds[-1])
    assert rc == _lib.NSOF_OK and total > 1000
    x, y = (torch.full((total,), -7, dtype=torch.int16, device=torch_dev) for _ in range(2))
    p = torch.full((total,), -7, dtype=torch.int8, device=torch_dev)
    t = torch.full((total,), -7, dtype=torch.int64, device=torch_dev)
    lut = nsof_lib.linear_response()
    torch.cuda.synchronize()

    def emit(capacity, frame_bounds):
        return ctx._lib.nsof_events_from_frames_emit_dev(ctx.ptr, d.data_ptr(), d.stride(1), d.stride(0), 5, 37, 53, UNEVEN.ctypes.data,
                                                         lut.ctypes.data, 2560, 2560, None, None, 0, frame_bounds.ctypes.data, 0, 1, -1,
                                                         capacity, x.data_ptr(), y.data_ptr(), p.data_ptr(), t.data_ptr(), None)
    assert emit(total - 1, bounds) == _lib.NSOF_EINVAL
    # bounds of another call: the emit pass forms the total itself and writes nothing when it differs
    assert emit(total, bounds - (bounds > 0)) == _lib.NSOF_OK
    ctx.synchronize()
    assert all(bool((v == -7).all()) for v in (x, y, p, t))
    assert emit(total, bounds) == _lib.NSOF_OK
    ctx.synchronize()
    want = events_from_frames_ref(random_frames, UNEVEN, 2560, 2560, timestamps="frame")
    assert np.array_equal(x.cpu().numpy(), want["x"]) and np.array_equal(t.cpu().numpy(), want["t"])

    plane = np.full((37, 53, 2), 10.0)
    plane[20, 30, 1] = 0.0
    with pytest.raises(NsofValueError):
        nsof_lib.events_from_frames_dev(d, UNEVEN, threshold_maps=plane, ctx=ctx)
    rc, bounds = _count(nsof_lib, ctx, d, UNEVEN, 1, 1, _dev((plane * 256).astype(np.int32), torch_dev))
    assert rc == _lib.NSOF_EINVAL and (bounds == -1).all()


def _c_args(d, **over):
    """The arguments of the two C entries for the 5 x 37 x 53 stack d, as a dict the cases below vary.  Host arrays are kept
    in the dict, so they live as long as the call."""
    a = dict(frames=d.data_ptr(), row_stride=d.stride(1), frame_stride=d.stride(0), n=5, h=37, w=53, times=UNEVEN.copy(),
             lut=np.arange(256, dtype=np.int32) * 256, c_on=2560, c_off=2560, plane=None, ref_in=None, ref_mode=0,
             bounds=np.full(6, -1, np.int64), mode=0, p_on=1, p_off=-1, capacity=None)
    a.update(over)
    return a


def _ptr(v):
    return v if v is None or isinstance(v, int) else v.ctypes.data


def _c_count(ctx, a):
    rc = ctx._lib.nsof_events_from_frames_count_dev(ctx.ptr, a["frames"], a["row_stride"], a["frame_stride"], a["n"], a["h"], a["w"],
                                                    _ptr(a["times"]), _ptr(a["lut"]), a["c_on"], a["c_off"], a["plane"], a["ref_in"],
                                                    a["ref_mode"], _ptr(a["bounds"]))
    return rc, ctx._lib.nsof_last_error(ctx.ptr).decode()


# what is wrong, the arguments changed, the status, what nsof_last_error must name
C_REFUSALS = [
    ("n 0", dict(n=0), "EINVAL", "0 frames of 53x37"),
    ("height 0", dict(h=0), "EINVAL", "5 frames of 53x0"),
    ("width above 32767", dict(w=32768), "EINVAL", "32768x37 is beyond the int16 coordinates"),
    ("height above 32767", dict(h=40000), "EINVAL", "53x40000 is beyond the int16 coordinates"),
    ("more than 2^24 frames", dict(n=(1 << 24) + 1), "EUNSUPPORTED", "16777217 frames are beyond one launch"),
    ("null frames", dict(frames=None), "EINVAL", "null pointer (d_frames)"),
    ("null times", dict(times=None), "EINVAL", "null pointer (times)"),
    ("null lut", dict(lut=None), "EINVAL", "null pointer (lut)"),
    ("null bounds", dict(bounds=None), "EINVAL", "null pointer (frame_bounds"),
    ("times equal", dict(times=np.array([0, 1000, 1000, 2100, 5000], np.int64)), "EINVAL", "times[2] = 1000 after times[1] = 1000"),
    ("times decrease", dict(times=np.array([0, 1000, 1700, 2100, 2099], np.int64)), "EINVAL", "times[4] = 2099 after times[3] = 2100"),
    ("a gap of 2^31", dict(times=np.array([0, 1000, 1700, 2100, 2100 + (1 << 31)], np.int64)), "EINVAL", "times[4] = 2147485748 after"),
    ("times across the int64 range", dict(times=np.array([-(1 << 62), 0, 1, 2, 1 << 62], np.int64)), "EINVAL", "times[1] = 0 after"),
    ("table entry above 2^30", dict(lut=np.r_[np.zeros(255, np.int32), np.int32((1 << 30) + 1)]), "EINVAL", "lut[255] = 1073741825 is outside"),
    ("table entry negative", dict(lut=np.r_[np.int32(0), np.int32(-1), np.zeros(254, np.int32)]), "EINVAL", "lut[1] = -1 is outside"),
    ("c_on 0", dict(c_on=0), "EINVAL", "thresholds c_on = 0, c_off = 2560"),
    ("c_off negative", dict(c_off=-5), "EINVAL", "thresholds c_on = 2560, c_off = -5"),
    ("ref_mode unknown", dict(ref_mode=3), "EINVAL", "ref_mode 3"),
    ("ref_mode given without a plane", dict(ref_mode=2), "EINVAL", "ref_mode 2 with d_ref_in NULL"),
    ("a reference plane in the zero mode", dict(ref_in="frames"), "EINVAL", "ref_mode 0 with d_ref_in given"),
]
C_EMIT_REFUSALS = [
    ("timestamps_mode unknown", dict(mode=2), "EINVAL", "timestamps_mode 2"),
    ("p_on beyond int8", dict(p_on=128), "EINVAL", "p_on = 128, p_off = -1 do not fit"),
    ("p_off beyond int8", dict(p_off=-129), "EINVAL", "p_on = 1, p_off = -129 do not fit"),
    ("capacity one short", dict(capacity=-1), "EINVAL", "is below the"),
    ("a total of 2^31 in the bounds", dict(bounds="2^31"), "EINVAL", "frame_bounds[5] = 2147483648 is not a total"),
    ("a negative total in the bounds", dict(bounds="negative"), "EINVAL", "frame_bounds[5] = -1 is not a total"),
    ("null x with events to write", dict(x=None), "EINVAL", "null pointer (d_x)"),
    ("null t with events to write", dict(t=None), "EINVAL", "null pointer (d_t)"),
]


@pytest.fixture(scope="module")
def c_stack(nsof_lib, ctx, torch_dev, random_frames):
    """The stack on the device, its bounds from the count entry, and output arrays filled with a mark."""
    import torch
    d = _dev(random_frames, torch_dev)
    torch.cuda.synchronize()
    a = _c_args(d)
    rc, _ = _c_count(ctx, a)
    assert rc == 0 and a["bounds"][-1] > 1000
    total = int(a["bounds"][-1])
    out = dict(x=torch.full((total,), -7, dtype=torch.int16, device=torch_dev), y=torch.full((total,), -7, dtype=torch.int16, device=torch_dev),
               p=torch.full((total,), -7, dtype=torch.int8, device=torch_dev), t=torch.full((total,), -7, dtype=torch.int64, device=torch_dev),
               ref=torch.full((37, 53), -7, dtype=torch.int32, device=torch_dev))
    torch.cuda.synchronize()
    return d, a["bounds"].copy(), out


@pytest.mark.parametrize("what,over,status,message", C_REFUSALS, ids=[r[0] for r in C_REFUSALS])
@pytest.mark.parametrize("entry", ["count", "emit"])
def test_c_entries_refuse_before_any_launch(nsof_lib, ctx, c_stack, entry, what, over, status, message):
    """ef_check, which both entries run first: the status, the value named in nsof_last_error, and nothing written."""
    from nsof import _lib
    d, bounds, out = c_stack
    over = dict(over)
    if over.get("ref_in") == "frames":
        over["ref_in"] = d.data_ptr()
    if entry == "emit" and what == "null bounds":
        message = "null pointer (frame_bounds)"
    a = _c_args(d, **over)
    if entry == "count":
        rc, msg = _c_count(ctx, a)
        assert a["bounds"] is None or (a["bounds"] == -1).all()
    else:
        if a["bounds"] is not None:
            a["bounds"] = bounds.copy()
        rc, msg = _c_emit(ctx, a, out, int(bounds[-1]))
    assert rc == getattr(_lib, "NSOF_" + status) and message in msg, (rc, msg)
    ctx.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())


@pytest.mark.parametrize("what,over,status,message", C_EMIT_REFUSALS, ids=[r[0] for r in C_EMIT_REFUSALS])
def test_c_emit_entry_refuses_before_any_launch(nsof_lib, ctx, c_stack, what, over, status, message):
    from nsof import _lib
    d, bounds, out = c_stack
    over, total = dict(over), int(bounds[-1])
    use = dict(out)
    for k in ("x", "t"):
        if k in over:
            use[k] = over.pop(k)
    b = bounds.copy()
    if isinstance(over.get("bounds"), str):
        b[-1] = 1 << 31 if over.pop("bounds") == "2^31" else -1
    capacity = total + over.pop("capacity", 0)
    a = _c_args(d, bounds=b, **over)
    rc, msg = _c_emit(ctx, a, use, capacity)
    assert rc == getattr(_lib, "NSOF_" + status) and message in msg, (rc, msg)
    ctx.synchronize()
    assert all(bool((v == -7).all()) for v in out.values())


def _c_emit(ctx, a, out, capacity):
    dp = lambda v: None if v is None else v.data_ptr()  # noqa: E731
    rc = ctx._lib.nsof_events_from_frames_emit_dev(ctx.ptr, a["frames"], a["row_stride"], a["frame_stride"], a["n"], a["h"], a["w"],
                                                   _ptr(a["times"]), _ptr(a["lut"]), a["c_on"], a["c_off"], a["plane"], a["ref_in"],
                                                   a["ref_mode"], _ptr(a["bounds"]), a["mode"], a["p_on"], a["p_off"], capacity,
                                                   dp(out["x"]), dp(out["y"]), dp(out["p"]), dp(out["t"]), dp(out["ref"]))
    return rc, ctx._lib.nsof_last_error(ctx.ptr).decode()


def test_own_temporaries_outlive_the_queued_kernels(nsof_lib, ctx, torch_dev, random_frames):
    """The uploaded threshold plane and the video entry's grey stack are read by kernels that are still queued when the emit
    entry returns.  Both calls wait for the context's stream before they let them go: blocks that torch's allocator hands
    out again at once are overwritten here right after the call, and the streams still equal the model's."""
    import torch
    from nsof import gating
    plane = np.random.default_rng(2).integers(200, 9000, (37, 53, 2))
    d = _dev(random_frames, torch_dev)
    got = nsof_lib.events_from_frames_dev(d, UNEVEN, threshold_maps=plane / 256.0, ctx=ctx)
    junk = [torch.full((37, 53, 2), 1, dtype=torch.int32, device=torch_dev) for _ in range(8)]   # the plane's size and type
    torch.cuda.synchronize()
    _assert_equal({k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got.items()},
                  events_from_frames_ref(random_frames, UNEVEN, plane[..., 0], plane[..., 1]))
    bgr = np.random.default_rng(4).integers(0, 256, (4, 21, 34, 3), dtype=np.uint8)
    gray = np.stack([gating.frame_to_gray(f, "BGR2GRAY") for f in bgr])
    got = nsof_lib.events_from_video_dev(_dev(bgr, torch_dev), frame_us=500, threshold=12.0, ctx=ctx)
    junk += [torch.full((4, 21, 34), 255, dtype=torch.uint8, device=torch_dev) for _ in range(8)]   # the grey stack's
    torch.cuda.synchronize()
    _assert_equal({k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in got.items()},
                  events_from_frames_ref(gray, np.arange(4, dtype=np.int64) * 500, units(12), units(12)))
    assert len(junk) == 16


def test_video_entry_goes_through_the_grey_conversion(nsof_lib, ctx, torch_dev):
    from nsof import gating
    bgr = np.random.default_rng(4).integers(0, 256, (4, 21, 34, 3), dtype=np.uint8)
    gray = np.stack([gating.frame_to_gray(f, "BGR2GRAY") for f in bgr])
    got = _host(nsof_lib.events_from_video_dev(_dev(bgr, torch_dev), frame_us=500, threshold=12.0, ctx=ctx), ctx)
    _assert_equal(got, events_from_frames_ref(gray, np.arange(4, dtype=np.int64) * 500, units(12), units(12)))


def test_video_to_flow_sequence_equals_the_event_pipeline_on_the_models_events(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import pipeline
    frames = drifting_texture(8, 64, 96)
    times = np.arange(8, dtype=np.int64) * 5000
    acc = dict(slice_us=1000, snapshot_every=5)
    surfaces, flows, ev = pipeline.video_to_flow_sequence(_dev(frames, torch_dev), frame_us=5000, threshold=10.0, p_off=0, ctx=ctx, **acc)
    want = events_from_frames_ref(frames, times, units(10), units(10), p_off=0)
    _assert_equal(_host(ev, ctx), want)
    assert len(want["x"]) > 10_000
    s_ref, f_ref = pipeline.events_to_flow_sequence(want["x"], want["y"], want["p"], want["t"], (64, 96), ctx=ctx, **acc)
    assert surfaces.shape[0] >= 2 and torch.equal(surfaces, s_ref) and torch.equal(flows, f_ref)
