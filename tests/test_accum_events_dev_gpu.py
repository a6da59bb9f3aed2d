"""GPU: the accumulators take event streams that lie in HBM -- bounds, check and staging on the device
(nsof_accum_slice_bounds_dev, nsof_accum_set_events_dev / _step_events_dev, nsof_accum_trials_step_dev) against the host
entries on the same streams (tests/accum_events_dev_cases.py).  Everything is array_equal: the device staging feeds the
kernels the host staging feeds, so not a bit may differ."""
import functools

import numpy as np
import pytest

import accum_events_dev_cases as K  # noqa: N812
from events_from_frames_ref import drifting_texture
from guard_bands import surrounded_in

pytestmark = pytest.mark.gpu

H, W = K.H, K.W
VOLTS = dict(active_v=-6.0, silent_v=0.0)
SNAP = 7


@functools.lru_cache(maxsize=None)
def _koff_plane():
    import nsof
    return nsof.variability_maps(H, W, dict(koff=0.1), seed=11)["koff"]


def _modes():
    return {"v1": dict(version=1), "v2_split": dict(version=2, polarity="split"), "v2_magnitude": dict(version=2, polarity="magnitude"),
            "v1_theta3": dict(version=1, theta_events=3), "v1_koff": dict(version=1, param_maps=dict(koff=_koff_plane()))}


MODES = ("v1", "v2_split", "v2_magnitude", "v1_theta3", "v1_koff")


def _dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)


def _tensors(name, dev):
    return tuple(_dev(v, dev) for v in K.stream(name))


def _acc(nsof, ctx, mode, **kw):
    return nsof.Accumulator(H, W, ctx=ctx, **VOLTS, **_modes()[mode], **kw)


def _state(acc):
    out = []
    for which in range(2 if acc.split else 1):
        s = acc.state(which)
        out += [s["w"], s["next_ok"], np.int64(s["slice_counter"])]
    return out


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g, w), (what, i)


# ---- bounds -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", K.CASES)
def test_device_bounds_equal_the_host_bounds(nsof_lib, ctx, torch_dev, name):
    t = K.stream(name)[3]
    want = nsof_lib.accumulator.slice_index_array(t, K.SLICE_US[name])
    got = nsof_lib.accumulator.slice_index_array(_dev(t, torch_dev), K.SLICE_US[name], ctx)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(want, K.yardstick(name))


def test_an_empty_device_stream_has_no_bounds(nsof_lib, ctx, torch_dev):
    import torch
    got = nsof_lib.accumulator.slice_index_array(torch.empty(0, dtype=torch.int64, device=torch_dev), 1000, ctx)
    assert got.shape == (0,)


@pytest.mark.parametrize("at", [(1,), (256,), (-1,), (256, 1023), (1023, -1)])
def test_a_decreasing_time_is_refused_and_the_first_one_named(nsof_lib, ctx, torch_dev, at):
    from nsof import _lib
    t = np.array(K.stream("blocky_1025")[3])
    n = len(t)
    t += np.arange(n) * 3          # strictly increasing, so that one lowered entry is one fault
    first = min(e % n for e in at)
    for e in at:
        t[e % n] = t[e % n - 1] - 1
    assert np.flatnonzero(np.diff(t) < 0)[0] + 1 == first
    with pytest.raises(nsof_lib.error, match=rf"t\[{first}\] < t\[{first - 1}\]") as e:
        nsof_lib.accumulator.slice_index_array(_dev(t, torch_dev), 1000, ctx)
    assert isinstance(e.value, ValueError) and e.value.status == _lib.NSOF_EINVAL
    # the context goes on working
    ok = K.stream("blocky_1025")[3]
    assert np.array_equal(nsof_lib.accumulator.slice_index_array(_dev(ok, torch_dev), 1000, ctx), K.yardstick("blocky_1025"))


# ---- one accumulator ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", K.STAGED)
def test_step_on_device_tensors_equals_step_on_host_arrays(nsof_lib, ctx, torch_dev, name, mode):
    ev, b = K.stream(name), K.yardstick(name)
    host, dev = _acc(nsof_lib, ctx, mode), _acc(nsof_lib, ctx, mode)
    try:
        host.step(*ev, b, snap_every=SNAP)
        dev.step(*_tensors(name, torch_dev), b, snap_every=SNAP)
        assert host.snapshot_count() == dev.snapshot_count() == (len(b) - 2) // SNAP + 1
        _same(_state(dev), _state(host), "state")
        _same(dev.snapshots(), host.snapshots(), "snapshots")
        if mode != "v1_theta3" or name == "dense":   # (three events of a slice at one pixel: the dense stream's hot pixels)
            assert _state(host)[0].std() > 0
    finally:
        host.close()
        dev.close()


@pytest.mark.parametrize("path", ("tiles", "copy_patch"))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", K.STAGED)
def test_set_events_on_device_tensors_feeds_every_run(nsof_lib, ctx, torch_dev, name, mode, path):
    """run over two sub-ranges, run_surface, then run_frames over the rest: slices [0, 3), [3, 7), [7, 10), then frames of
    5 slices each -- with W = 64 scheme 1's uniform array takes the tile walk unless copy + patch is asked for."""
    import torch
    ev, b = K.stream(name), K.yardstick(name)
    n_frames = (len(b) - 1 - 10) // 5
    assert n_frames >= 2
    out = []
    for stream in (ev, _tensors(name, torch_dev)):
        acc = _acc(nsof_lib, ctx, mode, frames_path=path)
        try:
            acc.set_events(*stream, b)
            assert acc.n_staged == len(b) - 1
            acc.run(0, 3)
            acc.run(3, 4, snap_every=2)
            got = _state(acc)
            surface = torch.zeros((H, W), dtype=torch.uint8, device=torch_dev)
            frames = torch.zeros((n_frames, H, W), dtype=torch.uint8, device=torch_dev)
            torch.cuda.synchronize()
            acc.run_surface(7, 3, surface)
            acc.run_frames(10, n_frames, 5, frames)
            got += _state(acc) + acc.snapshots() + [surface.cpu().numpy(), frames.cpu().numpy()]
        finally:
            acc.close()
        out.append(got)
    _same(out[1], out[0], "device vs host staging")
    if mode != "v1_theta3" or name == "dense":
        assert len(np.unique(out[0][-1])) > 1


@pytest.mark.parametrize("mode", ("v1", "v2_split"))
def test_bounds_that_start_inside_the_stream(nsof_lib, ctx, torch_dev, mode):
    ev, b = K.stream("dense"), K.yardstick("dense")[5:]
    assert b[0] > 0
    host, dev = _acc(nsof_lib, ctx, mode), _acc(nsof_lib, ctx, mode)
    try:
        host.set_events(*ev, b)
        dev.set_events(*_tensors("dense", torch_dev), b)
        for acc in (host, dev):
            acc.run(0, len(b) - 1, snap_every=SNAP)
        _same(_state(dev) + dev.snapshots(), _state(host) + host.snapshots(), "e0 > 0")
    finally:
        host.close()
        dev.close()


# ---- the trial accumulator ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("version,polarity", [(1, "split"), (2, "split")])
@pytest.mark.parametrize("cuts", [(), (13, 33)])
def test_trial_accumulator_on_device_tensors(nsof_lib, ctx, torch_dev, cuts, version, polarity):
    import torch
    ev, b = K.stream("dense"), K.yardstick("dense")
    maps = nsof_lib.variability_maps(H, W, dict(koff=0.1, kon=0.05), seed=5, trials=4)
    edges = (0,) + cuts + (len(b) - 1,)
    out = []
    for stream in (ev, _tensors("dense", torch_dev)):
        acc = nsof_lib.TrialAccumulator(H, W, maps, version, polarity, **VOLTS, c2c=dict(sigma=0.05, seed=3), snapshot_every=SNAP,
                                        memsize=16, ctx=ctx)
        try:
            cur = [acc.step(*stream, b[lo:hi + 1]) for lo, hi in zip(edges[:-1], edges[1:])]
            ctx.synchronize()
            got = [acc.w_dev(), torch.cat(cur, dim=2), acc.surface_u8_dev()]
            ctx.synchronize()
            out.append([v.cpu().numpy() for v in got])
        finally:
            acc.close()
    assert out[0][0].shape == (2 if version == 2 else 1, 4, H, W) and out[0][1].shape[2] == (len(b) - 2) // SNAP + 1
    _same(out[1], out[0], "trials")
    assert not np.array_equal(out[0][0][0, 0], out[0][0][0, 1])


def test_simulate_trials_dev_takes_a_device_stream(nsof_lib, ctx, torch_dev):
    ev = K.stream("gaps")
    maps = nsof_lib.variability_maps(H, W, dict(koff=0.1), seed=2, trials=3)
    kw = dict(version=2, slice_us=1000, sensor_size=(H, W), memsize=16, snapshot_every=5, ctx=ctx, **VOLTS)
    want = nsof_lib.simulate_trials_dev(ev, maps, **kw)
    got = nsof_lib.simulate_trials_dev(_tensors("gaps", torch_dev), maps, **kw)
    assert sorted(got) == sorted(want) == ["block_current", "resistance", "w"]
    for k in want:
        assert np.array_equal(got[k].cpu().numpy(), want[k].cpu().numpy()), k


# ---- refusals -----------------------------------------------------------------------------------------------------------

def _spoil(name, faults):
    """The stream with the coordinates of `faults` = [(event, array 0 / 1, value)] replaced."""
    x, y, p, t = (np.array(v) for v in K.stream(name))
    for e, which, value in faults:
        (x, y)[which][e] = value
    return x, y, p, t


FAULTS = [[(0, 0, W)], [(256, 1, H)], [(-1, 0, -1)], [(0, 1, -1)], [(256, 0, -1)], [(-1, 1, H)], [(256, 1, H), (1000, 0, W)],
          [(1024, 0, W), (255, 1, -1)]]


@pytest.mark.parametrize("faults", FAULTS)
@pytest.mark.parametrize("entry", ("step", "set_events", "trials"))
def test_a_coordinate_outside_the_sensor_is_refused_like_on_the_host(nsof_lib, ctx, torch_dev, faults, entry):
    from nsof import _lib
    name = "blocky_1025"
    bad, b = _spoil(name, faults), K.yardstick(name)
    first = min(e % 1025 for e, _, _ in faults)

    def call(acc, stream):
        if entry == "trials":
            return acc.step(*stream, b)
        return acc.step(*stream, b, snap_every=SNAP) if entry == "step" else acc.set_events(*stream, b)

    def make():
        if entry == "trials":
            return nsof_lib.TrialAccumulator(H, W, None, trials=2, **VOLTS, ctx=ctx)
        return _acc(nsof_lib, ctx, "v1")
    messages = []
    for stream in (bad, tuple(_dev(v, torch_dev) for v in bad)):
        acc = make()
        try:
            with pytest.raises(nsof_lib.error, match=rf"event {first} at \(") as e:
                call(acc, stream)
            assert isinstance(e.value, ValueError) and e.value.status == _lib.NSOF_EINVAL
            messages.append(str(e.value))
        finally:
            acc.close()
    assert messages[0] == messages[1] and f"outside the {W}x{H} sensor" in messages[0]


def test_a_refused_call_leaves_the_accumulator_and_its_staged_stream_alone(nsof_lib, ctx, torch_dev):
    good, b = K.stream("dense"), K.yardstick("dense")
    bad, bb = _spoil("blocky_1025", [(700, 0, W)]), K.yardstick("blocky_1025")
    twin, acc = _acc(nsof_lib, ctx, "v2_split"), _acc(nsof_lib, ctx, "v2_split")
    try:
        for a in (twin, acc):
            a.set_events(*(_tensors("dense", torch_dev) if a is acc else good), b)
            a.run(0, 15, snap_every=SNAP)
        before, count = _state(acc), acc.snapshot_count()
        assert count == 3
        for call in (lambda s: acc.set_events(*s, bb), lambda s: acc.step(*s, bb, snap_every=1)):
            with pytest.raises(nsof_lib.error, match="event 700 at"):
                call(tuple(_dev(v, torch_dev) for v in bad))
            _same(_state(acc), before, "state after a refused call")
            assert acc.snapshot_count() == count
        # bounds beyond the device stream are refused as well
        with pytest.raises(nsof_lib.error, match="shorter than the slice bounds"):
            acc.set_events(*(v[:100] for v in _tensors("dense", torch_dev)), b)
        # the stream staged before the refused calls is still there
        for a in (twin, acc):
            a.run(15, len(b) - 1 - 15, snap_every=SNAP)
        _same(_state(acc) + acc.snapshots(), _state(twin) + twin.snapshots(), "run after a refused call")
    finally:
        twin.close()
        acc.close()


def test_the_library_refuses_bounds_outside_the_device_stream(nsof_lib, ctx, torch_dev):
    from nsof import _lib
    from nsof.context import dev_ptr
    x, y, p, t = _tensors("blocky_255", torch_dev)
    acc = _acc(nsof_lib, ctx, "v1")
    try:
        for bounds in ([0, 100, 256], [-1, 100]):
            b = np.array(bounds, np.int64)
            rc = ctx._lib.nsof_accum_set_events_dev(acc._p, dev_ptr(x), dev_ptr(y), dev_ptr(p), dev_ptr(t), 255, b.ctypes.data, len(b) - 1)
            assert rc == _lib.NSOF_EINVAL and b"outside the 255 events" in ctx._lib.nsof_last_error(ctx.ptr)
        b = np.array([0, 100, 255], np.int64)
        assert ctx._lib.nsof_accum_set_events_dev(acc._p, dev_ptr(x), dev_ptr(y), None, dev_ptr(t), 255, b.ctypes.data, 2) == _lib.NSOF_OK
    finally:
        acc.close()


def test_python_refuses_what_is_no_device_stream(nsof_lib, ctx, torch_dev):
    import torch
    x, y, p, t = _tensors("blocky_257", torch_dev)
    hx, hy, hp, ht = K.stream("blocky_257")
    b = K.yardstick("blocky_257")
    t2 = torch.stack([t, t], dim=1)[:, 0]
    assert not t2.is_contiguous()
    bad = {"mixed host and device": (hx, y, p, t), "a CPU tensor among CUDA ones": (x, y, torch.from_numpy(np.array(hp)), t),
           "an int32 x": (x.to(torch.int32), y, p, t), "a non-contiguous t": (x, y, p, t2), "a shorter p": (x, y, p[:-1], t),
           "a list among CUDA tensors": (x, list(hy), p, t)}
    acc = _acc(nsof_lib, ctx, "v1")
    tri = nsof_lib.TrialAccumulator(H, W, None, trials=2, **VOLTS, ctx=ctx)
    try:
        before = _state(acc)
        for what, stream in bad.items():
            for call in (lambda s: acc.step(*s, b), lambda s: acc.set_events(*s, b), lambda s: tri.step(*s, b),
                         lambda s: nsof_lib.simulate_trials_dev(s, None, trials=2, sensor_size=(H, W), ctx=ctx)):
                with pytest.raises(nsof_lib.error) as e:
                    call(stream)
                assert isinstance(e.value, ValueError), what
        _same(_state(acc), before, "state after the refusals")
        for v in (t.to(torch.int32), t2, t[None]):
            with pytest.raises(nsof_lib.error, match="contiguous one-dimensional int64"):
                nsof_lib.accumulator.slice_index_array(v, 1000, ctx)
        with pytest.raises(nsof_lib.error, match="sensor_size"):
            nsof_lib.simulate_trials_dev((x, y, p, t), None, trials=2, ctx=ctx)
    finally:
        acc.close()
        tri.close()


# ---- guard bands --------------------------------------------------------------------------------------------------------

def _bytes_of(view):
    import torch
    raw = torch.empty(0, dtype=torch.uint8, device=view.device).set_(view.untyped_storage())
    return raw.cpu().numpy().copy()


@pytest.mark.parametrize("mode", ("v1", "v2_split"))
def test_nothing_outside_the_staged_events_is_read_and_no_input_is_written(nsof_lib, ctx, torch_dev, mode):
    """The four arrays sit inside larger allocations whose bands hold coordinates outside the sensor and wild times, and so do
    the events of the arrays themselves outside [e0, e1): the staged result is that of the clean host stream, whatever the
    poison, and every byte of the inputs survives the call."""
    import torch
    ev, full = K.stream("dense"), K.yardstick("dense")
    b = full[4:31]
    e0, e1 = int(b[0]), int(b[-1])
    assert 0 < e0 < e1 < len(ev[0])
    host = _acc(nsof_lib, ctx, mode)
    try:
        host.step(*ev, b, snap_every=SNAP)
        want = _state(host) + host.snapshots()
    finally:
        host.close()
    for poison in ((W, -1, 5, 2**62), (-300, 32767, -128, -2**62)):
        views = []
        for a, bad in zip(ev, poison):
            a = np.array(a)
            a[:e0] = bad
            a[e1:] = bad
            views.append(surrounded_in(torch, torch_dev, a[None], a.dtype.type(bad), offset_elems=3)[0])
        assert all(v.dim() == 1 and v.is_contiguous() for v in views)
        before = [_bytes_of(v) for v in views]
        acc = _acc(nsof_lib, ctx, mode)
        try:
            acc.step(*views, b, snap_every=SNAP)
            _same(_state(acc) + acc.snapshots(), want, f"poison {poison}")
        finally:
            acc.close()
        for u, v in zip(before, views):
            assert np.array_equal(u, _bytes_of(v))
        # the bounds entry reads t alone, and only its n entries
        clean = surrounded_in(torch, torch_dev, np.array(ev[3])[None], np.int64(poison[3]), offset_elems=1)[0]
        keep = _bytes_of(clean)
        assert np.array_equal(nsof_lib.accumulator.slice_index_array(clean, 1000, ctx), full)
        assert np.array_equal(keep, _bytes_of(clean))


# ---- pipelines ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _stream_96x64():
    from nsof import synth
    return synth.make_events(9, 96, 64, 6000, 40_000, box=(16, 12))


def test_events_to_flow_sequence_on_device_tensors(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import pipeline
    ev = _stream_96x64()
    kw = dict(slice_us=1000, snapshot_every=5, ctx=ctx)
    want = pipeline.events_to_flow_sequence(*ev, (64, 96), **kw)
    got = pipeline.events_to_flow_sequence(*(_dev(v, torch_dev) for v in ev), (64, 96), **kw)
    assert want[0].shape[0] >= 4 and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_events_to_roi_flows_on_device_tensors(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import gating, pipeline
    ev = _stream_96x64()
    cfg = gating.GatingConfig(MEMSIZE=8)
    kw = dict(slice_us=1000, snapshot_every=5, ctx=ctx)
    want = pipeline.events_to_roi_flows(*ev, (64, 96), cfg, **kw)
    got = pipeline.events_to_roi_flows(*(_dev(v, torch_dev) for v in ev), (64, 96), cfg, **kw)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and torch.equal(got[2], want[2])


@pytest.mark.parametrize("denoise", (None, dict(dt_us=3000, radius=2, min_support=3)))
def test_video_to_flow_sequence_brings_no_event_to_the_host(nsof_lib, ctx, torch_dev, monkeypatch, denoise):
    import torch
    from nsof import pipeline
    frames = _dev(drifting_texture(8, 64, 96), torch_dev)
    gen = dict(frame_us=5000, threshold=10.0, p_off=0)
    acc = dict(slice_us=1000, snapshot_every=5)
    # the host-array composition first: it downloads the stream, as the pipeline itself did
    raw = nsof_lib.events_from_frames_dev(frames, ctx=ctx, **gen)
    if denoise is not None:
        raw = nsof_lib.events_denoise_dev(raw["x"], raw["y"], raw["p"], raw["t"], (64, 96), bounds=raw["frame_bounds"], ctx=ctx, **denoise)
    ctx.synchronize()
    host = [raw[k].cpu().numpy() for k in "xypt"]
    s_ref, f_ref = pipeline.events_to_flow_sequence(*host, (64, 96), ctx=ctx, **acc)
    to_cpu = torch.Tensor.cpu

    def guarded(self, *a, **k):
        assert self.dtype not in (torch.int16, torch.int8, torch.int64), "an event array was copied to the host"
        return to_cpu(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "cpu", guarded)
    surfaces, flows, ev = pipeline.video_to_flow_sequence(frames, denoise=denoise, ctx=ctx, **gen, **acc)
    monkeypatch.undo()
    assert len(host[0]) > 1000 and surfaces.shape[0] >= 2
    assert torch.equal(surfaces, s_ref) and torch.equal(flows, f_ref)
    for k, v in zip("xypt", host):
        assert np.array_equal(ev[k].cpu().numpy(), v), k
