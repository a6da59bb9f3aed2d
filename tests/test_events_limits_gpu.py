"""GPU: events_from_frames_dev on the limit cases of tests/events_limits_cases.py -- coordinates up to 32766, more than 256
workgroups, 33-bit sort keys and negative times, stamp products beyond 2^53, a reference plane 2^31 and more from the frame,
the noise counter's carry, both sides of the 2^20 crossings of a walk, times at the top of the int64 range -- against the
restatements (whose preconditions and whose own arithmetic tests/test_events_limits_cpu.py checks).  Everything is integer:
x, y, p, t, frame_bounds, ref and, for the sensor entries, t_ok must be equal, no tolerance; every case runs twice and must give
the same bits."""
import numpy as np
import pytest

import events_limits_cases as L  # noqa: N812

pytestmark = pytest.mark.gpu

DTYPES = dict(x=np.int16, y=np.int16, p=np.int8, t=np.int64, frame_bounds=np.int64, ref=np.int32, t_ok=np.int64)


def _dev(a, torch_dev):
    import torch
    return torch.from_numpy(np.array(a)).to(torch_dev)   # a copy: the cases' arrays are read-only


def _host(res, ctx):
    ctx.synchronize()
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in res.items()}


def _call(nsof, ctx, torch_dev, frames, times, dev_kw, **over):
    kw = dict(dev_kw, **over)
    if isinstance(kw.get("ref"), np.ndarray):
        kw["ref"] = _dev(kw["ref"], torch_dev)
    d = frames if not isinstance(frames, np.ndarray) else _dev(frames, torch_dev)
    return _host(nsof.events_from_frames_dev(d, times, ctx=ctx, **kw), ctx)


def _assert_equal(got, want, keys, what=""):
    assert sorted(got) == sorted(keys), (what, sorted(got))
    for k in keys:
        assert got[k].dtype == DTYPES[k], (what, k, got[k].dtype)
    assert np.array_equal(got["frame_bounds"], want["frame_bounds"]), (what, "frame_bounds", got["frame_bounds"], want["frame_bounds"])
    for k in keys:
        assert np.array_equal(got[k], want[k]), (what, k)


def _keys(res):
    return ("x", "y", "p", "t", "frame_bounds", "ref") + (("t_ok",) if L.is_sensor(res) else ())


def _check(nsof_lib, ctx, torch_dev, name):
    _, frames, times, dev_kw, res = L.case(name)
    want = L.restatement(name)
    got = _call(nsof_lib, ctx, torch_dev, frames, times, dev_kw)
    _assert_equal(got, want, _keys(res), name)
    again = _call(nsof_lib, ctx, torch_dev, frames, times, dev_kw)
    _assert_equal(again, got, _keys(res), name + ", the second run")


@pytest.mark.parametrize("name", L.names("A"))
def test_coordinates_up_to_32766_and_353_workgroups(nsof_lib, ctx, torch_dev, name):
    """1 x 32767 and 32767 x 1 (every bit of the 15-bit coordinate fields of the reorder's packed word, the int16 outputs up to
    32766; the wide frame through the sensor entries too) and 300 x 301: 353 workgroups, so that the scan of a table row
    carries from its first 256-entry chunk into the second."""
    _check(nsof_lib, ctx, torch_dev, name)


@pytest.mark.parametrize("name", L.names("B"))
def test_a_33_bit_key_and_negative_times(nsof_lib, ctx, torch_dev, name):
    """Times from -5e9 over 5.2e9 us: t - T[0] needs 33 bits of the radix sort, and the stamps change sign."""
    _check(nsof_lib, ctx, torch_dev, name)


@pytest.mark.parametrize("name", L.names("C"))
def test_stamp_products_beyond_2_to_the_53(nsof_lib, ctx, torch_dev, name):
    """Products num * dt of up to 61 bits.  The C-exact cases are those in which a quotient formed in double gives other
    stamps (the precondition in tests/events_limits_cases.py counts them)."""
    _check(nsof_lib, ctx, torch_dev, name)


@pytest.mark.parametrize("name", L.names("D"))
def test_a_reference_plane_nobody_produced(nsof_lib, ctx, torch_dev, name):
    """r anywhere in the int32 range, INT32_MIN and INT32_MAX included: |L - r| of 2^31 and more at frame 0."""
    _check(nsof_lib, ctx, torch_dev, name)


@pytest.mark.parametrize("name", L.names("E"))
def test_the_noise_counter_carries_into_its_third_word(nsof_lib, ctx, torch_dev, name):
    """first_frame = 2^32 - 3: frame 3 of the call is frame 2^32.  One shot, and cut before and at the carry frame: the two
    calls, the second with the first's ref and t_ok and first_frame + k, give the one-shot stream."""
    _check(nsof_lib, ctx, torch_dev, name)
    _, frames, times, dev_kw, _ = L.case(name)
    one = L.restatement(name)
    d = _dev(frames, torch_dev)
    first = dev_kw["first_frame"]
    for k in (2, 3):   # the second call starts at frame 2^32 - 1 (its frame 1 is the carry), or at the carry frame itself
        a = nsof_lib.events_from_frames_dev(d[:k + 1], times[:k + 1], ctx=ctx, **dev_kw)
        ctx.synchronize()
        b = _host(nsof_lib.events_from_frames_dev(d[k:], times[k:], ctx=ctx, **dict(dev_kw, ref=a["ref"], t_ok=a["t_ok"], first_frame=first + k)), ctx)
        a = _host(a, ctx)
        assert b["frame_bounds"][1] == 0
        for key in "xypt":
            assert np.array_equal(np.concatenate([a[key], b[key]]), one[key]), (name, k, key)
        assert np.array_equal(np.concatenate([a["frame_bounds"], a["frame_bounds"][-1] + b["frame_bounds"][2:]]), one["frame_bounds"]), (name, k)
        assert np.array_equal(b["ref"], one["ref"]) and np.array_equal(b["t_ok"], one["t_ok"]), (name, k)


@pytest.mark.parametrize("name", L.names("F"))
def test_the_longest_step_a_walk_takes_and_the_same_step_without_a_walk(nsof_lib, ctx, torch_dev, name):
    """One pixel, one step: 2^20 - 1 crossings under a linear walk (a million events from one thread, each stamped by a 64-bit
    division and tested against t_ok), and 2^20 crossings where nothing is walked one by one: frame stamps (one survives), or
    no refractory time and no t_ok (all 2^20 survive).  The one slow case of the file: on an MI355X F-below-linear takes 2.9 s
    (two runs and the restatement's million Python steps), F-at-linear-no-walk 0.9 s, F-at-frame 0.07 s; the existing
    test_the_long_walk_at_the_finest_threshold[linear] of tests/test_events_sensor_gpu.py takes 0.3 s in the same session."""
    _check(nsof_lib, ctx, torch_dev, name)


def test_a_step_of_exactly_2_to_the_20_crossings_is_refused_under_a_linear_walk(nsof_lib, ctx, torch_dev):
    """The other side of F-below-linear: one crossing more."""
    from nsof import _lib
    from nsof.errors import NsofValueError
    _, frames, times, dev_kw, res = L.F_REFUSED
    assert int(res["lut"][1]) // res["c_on"] == L.WALK_MAX and res["refractory_us"] == 1 and res["timestamps"] == "linear"
    with pytest.raises(NsofValueError, match=r"crosses 2\^20 thresholds or more in one step, beyond the refractory walk of linear time stamps") as e:
        nsof_lib.events_from_frames_dev(_dev(frames, torch_dev), times, ctx=ctx, **dev_kw)
    assert e.value.status == _lib.NSOF_EUNSUPPORTED
    ctx.synchronize()


@pytest.mark.parametrize("name", L.names("G"))
def test_times_at_the_top_of_the_int64_range(nsof_lib, ctx, torch_dev, name):
    """The sensor entries with times[n-1] == INT64_MAX - refractory_us, the last time they take: a pixel that fires at
    times[n-1] ends with t_ok == INT64_MAX.  The plain entries, and the sensor entries without a refractory time, with
    times[n-1] == INT64_MAX."""
    _check(nsof_lib, ctx, torch_dev, name)


def test_one_microsecond_later_the_sensor_entries_refuse_and_the_plain_entries_do_not(nsof_lib, ctx, torch_dev):
    from nsof import _lib
    from nsof.errors import NsofValueError
    _, frames, times, dev_kw, _ = L.case("G-sensor-linear")
    d = _dev(frames, torch_dev)
    with pytest.raises(NsofValueError, match=r"times_us\[3\] = \d+ with refractory_us = 700") as e:
        nsof_lib.events_from_frames_dev(d, times + 1, ctx=ctx, **dev_kw)
    assert e.value.status == _lib.NSOF_EINVAL
    plain = {k: v for k, v in dev_kw.items() if k not in ("refractory_us", "noise")}
    got = _call(nsof_lib, ctx, torch_dev, d, times + 1, plain)
    want = L.restate(frames, times + 1, dict(c_on=2560, c_off=2560, timestamps="linear"))
    _assert_equal(got, want, ("x", "y", "p", "t", "frame_bounds", "ref"))
