"""GPU: events_denoise_dev on every case of tests/events_denoise_cases.py against the sequential restatement (whose own
arithmetic and whose keep shares tests/test_events_denoise_cpu.py checks).  Everything is integer: keep, n_kept, the kept
x, y, p, t, bounds and last must be equal, no tolerance, in one call and in two; every case runs twice on one context and must
give the same bits.  Then the device-side refusals and the guard of the compact pass through the C entries on poisoned
outputs, the generator's stream through the filter, and the pipeline join."""
import ctypes as C

import numpy as np
import pytest

import events_denoise_cases as K  # noqa: N812
from events_denoise_ref import NEVER, denoise_result, denoise_walk
from events_from_frames_ref import drifting_texture

pytestmark = pytest.mark.gpu

DTYPES = dict(x=np.int16, y=np.int16, p=np.int8, t=np.int64, keep=np.uint8, bounds=np.int64, last=np.int64)
POISON = 0x5A


def _dev(a, torch_dev):
    import torch
    return torch.from_numpy(np.array(a)).to(torch_dev)   # a copy: the cases' arrays are read-only


def _host(res, ctx):
    ctx.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in res.items()}


def _run(nsof, ctx, torch_dev, name, lo=0, hi=None, last=None, bounds=None):
    c = K.CASES[name]
    ev = [_dev(v, torch_dev) for v in K.stream(name, lo, hi)]
    if isinstance(last, np.ndarray):
        last = _dev(last, torch_dev)
    return _host(nsof.events_denoise_dev(*ev, c["hw"], bounds=bounds, last=last, ctx=ctx, **c["kw"]), ctx)


def _assert_equal(got, want, what):
    assert sorted(got) == ["bounds", "keep", "last", "n_kept", "p", "t", "x", "y"], (what, sorted(got))
    assert got["n_kept"] == want["n_kept"], (what, got["n_kept"], want["n_kept"])
    for k, dtype in DTYPES.items():
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        assert got[k].dtype == dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


# the largest case first: the cases after it reuse a workspace that a larger call has left behind
ORDER = ("33x65",) + tuple(n for n in K.NAMES if n != "33x65")


@pytest.mark.parametrize("name", ORDER)
def test_one_call_equals_the_restatement_twice(nsof_lib, ctx, torch_dev, name):
    c, want = K.CASES[name], K.want(name)
    got = _run(nsof_lib, ctx, torch_dev, name, last=c["last"], bounds=c["bounds"])
    _assert_equal(got, want, name)
    again = _run(nsof_lib, ctx, torch_dev, name, last=c["last"], bounds=c["bounds"])
    _assert_equal(again, got, name + ", the second run")
    no_bounds = _run(nsof_lib, ctx, torch_dev, name, last=c["last"])
    _assert_equal(no_bounds, dict(want, bounds=None), name + ", without bounds")


@pytest.mark.parametrize("name", [n for n in ORDER if K.CASES[n]["cuts"]])
def test_two_calls_equal_one(nsof_lib, ctx, torch_dev, name):
    """Events [0, k) and then [k, N) from the first call's last, for every cut of the case (a third of the stream, inside a run
    of equal t, before the first event, after the last): the mask, the kept stream, the bounds and the final last of one call."""
    c, want = K.CASES[name], K.want(name)
    for cut in c["cuts"]:
        b_first, b_second = c["bounds"][c["bounds"] <= cut], c["bounds"][c["bounds"] > cut] - cut
        for rerun in range(2):
            a = _run(nsof_lib, ctx, torch_dev, name, 0, cut, c["last"], b_first)
            b = _run(nsof_lib, ctx, torch_dev, name, cut, None, a["last"], b_second)
            for k in ("keep", "x", "y", "p", "t"):
                assert np.array_equal(np.concatenate([a[k], b[k]]), want[k]), (name, cut, k, rerun)
            assert a["n_kept"] + b["n_kept"] == want["n_kept"]
            assert np.array_equal(np.concatenate([a["bounds"], a["n_kept"] + b["bounds"]]), want["bounds"]), (name, cut, rerun)
            assert np.array_equal(b["last"], want["last"]), (name, cut, rerun)
            assert np.array_equal(a["last"], K.walk(name, 0, cut)[1]), (name, cut, rerun)


def test_a_small_call_after_a_large_one_and_back(nsof_lib, ctx, torch_dev):
    for name in ("33x65", "n1", "hot-pixel", "n0-last", "5x7", "33x65"):
        c = K.CASES[name]
        _assert_equal(_run(nsof_lib, ctx, torch_dev, name, last=c["last"], bounds=c["bounds"]), K.want(name), name)


# ---- the C entries on poisoned outputs ---------------------------------------------------------------------------------
def _raw(nsof_lib, ctx, torch_dev, x, y, p, t, hw, kw, capacity=None, mark=True):
    """The two entries called by hand: every output is poisoned first.  Returns (rc of mark, n_kept as the host holds it, rc of
    compact, the outputs on the host).  capacity: what the compact entry is told (None: the mark entry's n_kept)."""
    import torch
    from nsof.context import dev_ptr
    lib = ctx._lib
    n = len(x)
    ev = [_dev(v, torch_dev) for v in (x, y, p, t)]
    c = 2 if kw.get("same_polarity") else 1
    out = dict(keep=torch.full((n,), POISON, dtype=torch.uint8, device=torch_dev),
               x=torch.full((n,), POISON, dtype=torch.int16, device=torch_dev), y=torch.full((n,), POISON, dtype=torch.int16, device=torch_dev),
               p=torch.full((n,), POISON, dtype=torch.int8, device=torch_dev), t=torch.full((n,), POISON, dtype=torch.int64, device=torch_dev),
               last=torch.full((c,) + tuple(hw), POISON, dtype=torch.int64, device=torch_dev))
    torch.cuda.synchronize(torch_dev)
    n_kept = C.c_int64(-7)
    stream = (ctx.ptr, *(dev_ptr(v) for v in ev), n, hw[0], hw[1])
    rc_mark = None
    if mark is True:
        rc_mark = lib.nsof_events_denoise_mark_dev(*stream, kw["dt_us"], kw.get("radius", 1), kw.get("min_support", 1),
                                                   int(kw.get("same_polarity", False)), int(kw.get("include_self", False)), None, None, 0,
                                                   dev_ptr(out["keep"]), C.byref(n_kept), None)
    if capacity is None:
        capacity = max(n_kept.value, 0)
    if isinstance(mark, np.ndarray):   # a keep array the caller made up
        out["keep"] = _dev(mark, torch_dev)
        torch.cuda.synchronize(torch_dev)
    rc_compact = lib.nsof_events_denoise_compact_dev(*stream, int(kw.get("same_polarity", False)), None, dev_ptr(out["keep"]), capacity,
                                                     *(dev_ptr(out[k]) for k in "xypt"), dev_ptr(out["last"]))
    ctx.synchronize()
    return rc_mark, n_kept.value, rc_compact, {k: v.cpu().numpy() for k, v in out.items()}


def _untouched(out, keys):
    for k in keys:
        assert (out[k] == POISON).all(), k


BAD = [
    ("x equal to W", dict(x=7), r"an event lies outside the 7x5 sensor"),
    ("y equal to H", dict(y=5), r"an event lies outside the 7x5 sensor"),
    ("a negative x", dict(x=-1), r"an event lies outside the 7x5 sensor"),
    ("a negative y", dict(y=-32768), r"an event lies outside the 7x5 sensor"),
    ("one decreasing t", dict(t="decrease"), r"t decreases somewhere in the stream"),
]


@pytest.mark.parametrize("what,bad,message", BAD, ids=[b[0] for b in BAD])
def test_device_side_refusals_write_nothing(nsof_lib, ctx, torch_dev, what, bad, message):
    """Input validation on the device: the mark entry returns NSOF_EINVAL and writes neither keep nor n_kept, the compact entry
    writes nothing; the Python call raises with the status.  Nothing faults: a refused event addresses nothing."""
    from nsof import _lib
    from nsof.errors import NsofValueError
    x, y, p, t = (np.array(v) for v in K.stream("5x7"))
    i = 1700
    if bad.get("t") == "decrease":
        t[i] = t[i - 1] - 1
    else:
        for k, v in bad.items():
            dict(x=x, y=y)[k][i] = v
    kw = K.CASES["5x7"]["kw"]
    rc_mark, n_kept, rc_compact, out = _raw(nsof_lib, ctx, torch_dev, x, y, p, t, (5, 7), kw, capacity=len(x) // 2)
    assert rc_mark == _lib.NSOF_EINVAL and n_kept == -7 and rc_compact == _lib.NSOF_OK
    _untouched(out, ("keep", "x", "y", "p", "t", "last"))
    with pytest.raises(NsofValueError, match=r"events_denoise_mark: " + message) as e:
        nsof_lib.events_denoise_dev(*(_dev(v, torch_dev) for v in (x, y, p, t)), (5, 7), ctx=ctx, **kw)
    assert e.value.status == _lib.NSOF_EINVAL
    ctx.synchronize()
    # the same context takes the good stream afterwards
    _assert_equal(_run(nsof_lib, ctx, torch_dev, "5x7", bounds=K.CASES["5x7"]["bounds"]), K.want("5x7"), "after " + what)


def test_a_compact_call_with_another_capacity_writes_nothing(nsof_lib, ctx, torch_dev):
    from nsof import _lib
    name = "33x65"
    c, want = K.CASES[name], K.want(name)
    ev = K.stream(name)
    for capacity in (want["n_kept"] - 1, want["n_kept"] + 1, 0, len(ev[0])):
        rc_mark, n_kept, rc_compact, out = _raw(nsof_lib, ctx, torch_dev, *ev, c["hw"], c["kw"], capacity=capacity)
        assert rc_mark == _lib.NSOF_OK and n_kept == want["n_kept"] and rc_compact == _lib.NSOF_OK
        assert np.array_equal(out["keep"], want["keep"])
        _untouched(out, ("x", "y", "p", "t", "last"))
    # a keep array of another stream with the true capacity of the first: its own count decides
    other = np.ones(len(ev[0]), np.uint8)
    _, _, rc_compact, out = _raw(nsof_lib, ctx, torch_dev, *ev, c["hw"], c["kw"], capacity=want["n_kept"], mark=other)
    assert rc_compact == _lib.NSOF_OK
    _untouched(out, ("x", "y", "p", "t", "last"))
    # ... and the capacity the mark entry returned writes the kept stream, the rest of the outputs untouched
    rc_mark, n_kept, rc_compact, out = _raw(nsof_lib, ctx, torch_dev, *ev, c["hw"], c["kw"])
    assert (rc_mark, rc_compact) == (_lib.NSOF_OK, _lib.NSOF_OK)
    for k in "xypt":
        assert np.array_equal(out[k][:n_kept], want[k]) and (out[k][n_kept:] == POISON).all(), k
    assert np.array_equal(out["last"], want["last"])


def test_the_c_entries_refuse_their_arguments_before_any_launch(nsof_lib, ctx, torch_dev):
    from nsof import _lib
    c = K.CASES["5x7"]
    ev = K.stream("5x7")
    for kw, message in ((dict(dt_us=-1), b"dt_us = -1 is outside [0, 2^31)"), (dict(dt_us=1 << 31), b"dt_us = 2147483648"),
                        (dict(dt_us=3, radius=3), b"radius = 3; 1 or 2 expected"), (dict(dt_us=3, min_support=10), b"min_support = 10 is outside [1, 9]"),
                        (dict(dt_us=3, min_support=0), b"min_support = 0 is outside [1, 9]")):
        rc_mark, n_kept, _, out = _raw(nsof_lib, ctx, torch_dev, *ev, c["hw"], kw, capacity=0)
        assert rc_mark == _lib.NSOF_EINVAL and n_kept == -7 and message in ctx._lib.nsof_last_error(ctx.ptr), kw
        _untouched(out, ("keep", "x", "y", "p", "t"))
    for hw in ((5, 32768), (0, 7)):
        rc_mark, n_kept, rc_compact, out = _raw(nsof_lib, ctx, torch_dev, *ev, hw, c["kw"], capacity=0)
        assert rc_mark == rc_compact == _lib.NSOF_EINVAL and b"sensor" in ctx._lib.nsof_last_error(ctx.ptr)
    rc_mark, n_kept, rc_compact, out = _raw(nsof_lib, ctx, torch_dev, *ev, c["hw"], c["kw"], capacity=len(ev[0]) + 1, mark=False)
    assert rc_compact == _lib.NSOF_EINVAL and b"capacity 3001 is not a kept count of 3000 events" in ctx._lib.nsof_last_error(ctx.ptr)
    _untouched(out, ("keep", "x", "y", "p", "t", "last"))


# ---- the generator's stream and the pipeline ---------------------------------------------------------------------------
SENSOR = dict(refractory_us=700, noise=dict(seed=31, rate_hz=8))
FILTER = dict(dt_us=4000, min_support=2, same_polarity=True)


def test_generator_then_filter_equals_the_restatement(nsof_lib, ctx, torch_dev):
    """A 48 x 64 video of 12 frames with noise and a refractory time: the filter takes the generator's tensors where they lie and
    its frame_bounds come through as the bounds of the kept stream."""
    frames = _dev(drifting_texture(12, 48, 64), torch_dev)
    ev = nsof_lib.events_from_frames_dev(frames, frame_us=33333, threshold=10.0, ctx=ctx, **SENSOR)
    got = _host(nsof_lib.events_denoise_dev(ev["x"], ev["y"], ev["p"], ev["t"], (48, 64), bounds=ev["frame_bounds"], ctx=ctx, **FILTER), ctx)
    x, y, p, t = (ev[k].cpu().numpy() for k in "xypt")
    keep, last = denoise_walk(x, y, p, t, 48, 64, **FILTER)
    assert len(x) > 5000 and 0.05 < keep.mean() < 0.95
    want = denoise_result(x, y, p, t, keep, last, ev["frame_bounds"])
    _assert_equal(got, want, "generator -> filter")
    assert got["bounds"].shape == (13,) and got["bounds"][-1] == got["n_kept"]
    for k in range(12):   # the kept events of frame k are those of the generator's frame k
        lo, hi = ev["frame_bounds"][k:k + 2]
        assert np.array_equal(got["t"][got["bounds"][k]:got["bounds"][k + 1]], t[lo:hi][keep[lo:hi] != 0]), k


def test_video_to_flow_sequence_with_the_filter_equals_the_composition(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import pipeline
    frames = _dev(drifting_texture(8, 64, 96), torch_dev)
    gen = dict(frame_us=5000, threshold=10.0, p_off=0)
    acc = dict(slice_us=1000, snapshot_every=5)
    sensor = dict(noise=dict(seed=21, rate_hz=30))
    flt = dict(dt_us=3000, radius=2, min_support=3)
    surfaces, flows, ev = pipeline.video_to_flow_sequence(frames, sensor=sensor, denoise=flt, ctx=ctx, **gen, **acc)
    raw = nsof_lib.events_from_frames_dev(frames, ctx=ctx, **gen, **sensor)
    kept = _host(nsof_lib.events_denoise_dev(raw["x"], raw["y"], raw["p"], raw["t"], (64, 96), bounds=raw["frame_bounds"], ctx=ctx, **flt), ctx)
    assert 0 < kept["n_kept"] < len(raw["x"])
    s_ref, f_ref = pipeline.events_to_flow_sequence(kept["x"], kept["y"], kept["p"], kept["t"], (64, 96), ctx=ctx, **acc)
    assert surfaces.shape[0] >= 2 and torch.equal(surfaces, s_ref) and torch.equal(flows, f_ref)
    ev = _host(ev, ctx)
    assert sorted(ev) == ["frame_bounds", "keep", "last", "n_kept", "p", "ref", "t", "t_ok", "x", "y"]
    for k in ("x", "y", "p", "t", "keep", "last"):
        assert np.array_equal(ev[k], kept[k]), k
    assert ev["n_kept"] == kept["n_kept"] and np.array_equal(ev["frame_bounds"], kept["bounds"])
    assert np.array_equal(ev["ref"], raw["ref"].cpu().numpy())
    # the filter changes what the accumulator sees
    s_raw, _ = pipeline.events_to_flow_sequence(*(raw[k].cpu().numpy() for k in "xypt"), (64, 96), ctx=ctx, **acc)
    assert not torch.equal(s_raw, surfaces)


def test_video_to_flow_sequence_without_the_filter_is_unchanged(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import pipeline
    frames = _dev(drifting_texture(8, 64, 96), torch_dev)
    gen = dict(frame_us=5000, threshold=10.0, p_off=0)
    acc = dict(slice_us=1000, snapshot_every=5)
    surfaces, flows, ev = pipeline.video_to_flow_sequence(frames, denoise=None, ctx=ctx, **gen, **acc)
    raw = _host(nsof_lib.events_from_frames_dev(frames, ctx=ctx, **gen), ctx)
    ev = _host(ev, ctx)
    assert sorted(ev) == sorted(raw) == ["frame_bounds", "p", "ref", "t", "x", "y"]
    for k in raw:
        assert np.array_equal(ev[k], raw[k]), k
    s_ref, f_ref = pipeline.events_to_flow_sequence(raw["x"], raw["y"], raw["p"], raw["t"], (64, 96), ctx=ctx, **acc)
    assert torch.equal(surfaces, s_ref) and torch.equal(flows, f_ref)
    assert NEVER == -2 ** 63
