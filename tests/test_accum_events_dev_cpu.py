"""CPU: the yardstick of the device-staging tests (the host bounds function is the reference script's searchsorted on every
case), the C ABI of the device entries, and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import accum_events_dev_cases as K  # noqa: N812

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nsof_accum_slice_bounds_dev", "nsof_accum_set_events_dev", "nsof_accum_step_events_dev", "nsof_accum_trials_step_dev")


@pytest.mark.parametrize("name", K.CASES)
def test_host_bounds_are_the_scripts_searchsorted(nsof_lib, name):
    t = K.stream(name)[3]
    assert (np.diff(t) >= 0).all() and np.abs(t).max() < 2**62
    got = nsof_lib.accumulator.slice_index_array(t, K.SLICE_US[name])
    want = K.yardstick(name)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert nsof_lib.accumulator.slice_index_array(list(t), K.SLICE_US[name], None).tolist() == want.tolist()


def test_the_cases_are_what_they_are_said_to_be():
    b = {name: K.yardstick(name) for name in K.CASES}
    n = {name: len(K.stream(name)[0]) for name in K.CASES}
    for name in K.STAGED:
        assert len(b[name]) - 1 >= 20, name
    x, y, p, t = K.stream("dense")
    assert n["dense"] == 6000 and t[-1] - t[0] < 40_000 and set(np.unique(p)) == {-1, 0, 1}
    s = np.searchsorted(b["dense"], np.arange(6000), side="right")
    keys = (s.astype(np.int64) * K.H + y) * K.W + x
    assert len(np.unique(keys)) < 6000                                   # duplicates per (pixel, slice)
    sizes = np.diff(b["gaps"])
    empty = "".join("0" if v == 0 else "1" for v in sizes)
    assert all(len(run) >= 3 for run in re.findall("0+", empty)) and empty.count("0") >= 9
    tg = K.stream("gaps")[3]
    assert any(v >= 1 and tg[lo] == tg[lo + v - 1] for lo, v in zip(b["gaps"][:-1], sizes))
    assert 1 in sizes and any(v > 1 and tg[lo] == tg[lo + v - 1] for lo, v in zip(b["gaps"][:-1], sizes))
    te = K.stream("exact")[3]
    assert (te[-1] - te[0]) % K.SLICE_US["exact"] == 0 and b["exact"][-1] < n["exact"]
    assert n["one"] == 1 and len(b["one"]) == 1 and len(b["same_time"]) == 1 and n["same_time"] > 1
    assert K.stream("neg")[3][0] <= -4_999_000 and len(b["sparse_us"]) > n["sparse_us"]
    assert [n[f"blocky_{k}"] for k in K.BLOCKY] == list(K.BLOCKY)


def test_the_device_entries_are_declared_and_bound(nsof_lib):
    from nsof import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "nsof.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)", code)
        assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    # the device twins take the host twins' arguments plus the number of events
    for host in ("nsof_accum_set_events", "nsof_accum_step_events", "nsof_accum_trials_step"):
        assert len(_lib.SIGNATURES[host + "_dev"][1]) == len(_lib.SIGNATURES[host][1]) + 1
    assert _lib.SIGNATURES["nsof_accum_slice_bounds_dev"][0] is C.c_int64


class _InHbm:
    """Reports what a CUDA tensor reports and is nothing else."""
    is_cuda = True


@pytest.fixture
def no_device(monkeypatch, nsof_lib):
    """Any attempt to make a context or to call the library fails the test."""
    from nsof import accumulator as A  # noqa: N812
    from nsof import context

    def refused(*a, **k):
        raise AssertionError("device work before the refusal")
    monkeypatch.setattr(A, "default_context", refused)
    monkeypatch.setattr(context, "default_context", refused)
    monkeypatch.setattr(A._lib, "load", refused)
    return nsof_lib


def test_a_device_stream_needs_the_sensor_size_before_any_context(no_device):
    nsof = no_device
    ev = tuple(_InHbm() for _ in range(4))
    for fn in (nsof.simulate_trials_dev, nsof.simulate_trials):
        with pytest.raises(nsof.error, match="sensor_size") as e:
            fn(ev, None, trials=2)
        assert isinstance(e.value, ValueError)
    # ... and with it, a stand-in that is no tensor is refused like any mix of host and device arrays: still no context
    with pytest.raises(nsof.error, match="CUDA tensor"):
        nsof.simulate_trials_dev(ev, None, trials=2, sensor_size=(K.H, K.W))
    x, y, p, t = K.stream("dense")
    with pytest.raises(nsof.error, match="x is no CUDA tensor"):
        nsof.simulate_trials_dev((x, y, p, _InHbm()), None, trials=2, sensor_size=(K.H, K.W))


def test_host_streams_are_not_taken_for_device_streams(nsof_lib):
    import torch
    A = nsof_lib.accumulator  # noqa: N806
    x, y, p, t = K.stream("dense")
    assert A.device_events("who", x, y, p, t) is None
    assert A.device_events("who", *(torch.from_numpy(v.copy()) for v in (x, y, p, t))) is None
    assert A.device_events("who", list(x), list(y), list(p), list(t)) is None
    assert np.array_equal(A.slice_index_array(torch.from_numpy(t.copy()), 1000), K.yardstick("dense"))
