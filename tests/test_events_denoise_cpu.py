"""CPU: the background-activity filter's restatements (tests/events_denoise_ref.py) against each other on every case of
tests/events_denoise_cases.py -- the int64 walk against the Python-int walk, the sorted-segment formulation against the walk,
two calls against one -- the keep shares of the random cases, and, without a device, the Python layer's refusals and the new
symbols."""
import os
import re

import numpy as np
import pytest

import events_denoise_cases as K  # noqa: N812
from conftest import ROOT
from events_denoise_ref import NEVER, denoise_result, denoise_sorted, denoise_walk_int

ARGS = {"nsof_events_denoise_mark_dev": 19, "nsof_events_denoise_compact_dev": 17}


def _same(a, b, what):
    assert a[0].dtype == b[0].dtype == np.uint8 and a[1].dtype == b[1].dtype == np.int64, what
    assert a[1].shape == b[1].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), what


@pytest.mark.parametrize("name", K.NAMES)
def test_the_int64_walk_equals_the_python_int_walk(name):
    c = K.CASES[name]
    _same(K.walk(name), denoise_walk_int(*K.stream(name), *c["hw"], last=c["last"], **c["kw"]), name)


@pytest.mark.parametrize("name", K.NAMES)
def test_the_sorted_segment_formulation_equals_the_walk(name):
    c = K.CASES[name]
    _same(K.walk(name), denoise_sorted(*K.stream(name), *c["hw"], last=c["last"], **c["kw"]), name)
    for cut in c["cuts"]:
        first = K.walk(name, 0, cut)
        _same(K.walk(name, cut, None, cut), denoise_sorted(*K.stream(name, cut), *c["hw"], last=first[1], **c["kw"]), (name, cut))


@pytest.mark.parametrize("name", K.NAMES)
def test_two_calls_equal_one(name):
    keep, last = K.walk(name)
    for cut in K.CASES[name]["cuts"]:
        a, b = K.walk(name, 0, cut), K.walk(name, cut, None, cut)
        assert np.array_equal(np.concatenate([a[0], b[0]]), keep) and np.array_equal(b[1], last), (name, cut)


def test_the_cuts_fall_where_they_should():
    for name, c in K.CASES.items():
        if name in ("5x7", "33x65", "9x4-dt0", "borders-r2", "300x301", "box-noise"):
            tie = c["cuts"][1]
            assert c["cuts"][0] == len(c["x"]) // 3 and c["t"][tie - 1] == c["t"][tie], name   # inside a run of equal t


def test_keep_shares():
    """Both outcomes are exercised: every random case keeps between 5 % and 95 % (1 x 1 without its own pixel: nothing)."""
    checked = 0
    for name, c in K.CASES.items():
        if c["share"] is not None:
            share = float(K.walk(name)[0].mean())
            assert c["share"][0] <= share <= c["share"][1], (name, share)
            checked += 1
    assert checked >= 15
    assert K.CASES["1x1-no-self"]["share"] == (0.0, 0.0) and not K.walk("1x1-no-self")[0].any()
    keep, noise = K.walk("box-noise")[0], K.CASES["box-noise"]["is_noise"]
    assert keep[noise].mean() < 0.05 and keep[~noise].mean() > 0.95   # what the filter is for


def test_state_properties():
    keep, last = K.walk("33x65")
    x, y, p, t = K.stream("33x65")
    want = np.full((2, 33, 65), NEVER, np.int64)
    want[(p <= 0).astype(int), y, x] = t   # later events overwrite earlier ones
    assert np.array_equal(last, want)
    res = denoise_result(x, y, p, t, keep, last, K.CASES["33x65"]["bounds"])
    assert res["bounds"][0] == 0 and res["bounds"][-1] == res["n_kept"] == len(res["x"]) == int(keep.sum())
    assert (np.diff(res["t"]) >= 0).all() and (np.diff(res["bounds"]) >= 0).all()
    # INT64_MIN is `never`: an event stamped INT64_MIN supports nothing, whatever dt_us
    keep, _ = K.walk("extreme-t-dt-max")
    assert K.stream("extreme-t-dt-max")[3][0] == NEVER and keep.any() and not keep.all()


def _good(n=3):
    import torch
    return [torch.zeros(n, dtype=d) for d in (torch.int16, torch.int16, torch.int8, torch.int64)]


# what is wrong, the positional overrides (index -> value), the keyword arguments, the status, what the message must name
REFUSALS = [
    ("x of another dtype", {0: "int32 [3]"}, {}, "EINVAL", r"x must be an int16 tensor \(got torch.int32\)"),
    ("p of another dtype", {2: "int16 [3]"}, {}, "EINVAL", r"p must be an int8 tensor"),
    ("t of another dtype", {3: "int32 [3]"}, {}, "EINVAL", r"t must be an int64 tensor"),
    ("y an array", {1: np.zeros(3, np.int16)}, {}, "EINVAL", r"y must be an int16 tensor"),
    ("t of another length", {3: "int64 [4]"}, {}, "ESHAPE", r"t must be contiguous, one-dimensional and as long as x \(got \(4,\), x \(3,\)\)"),
    ("y two-dimensional", {1: "int16 [3, 1]"}, {}, "ESHAPE", r"y must be contiguous, one-dimensional"),
    ("sensor_hw a number", {}, dict(sensor_hw=5), "ESHAPE", r"sensor_hw = 5; \(H, W\) expected"),
    ("sensor_hw beyond int16", {}, dict(sensor_hw=(4, 32768)), "ESHAPE", r"sensor_hw = 4x32768 is beyond the int16 coordinates"),
    ("sensor_hw of zero", {}, dict(sensor_hw=(0, 5)), "ESHAPE", r"sensor_hw = 0x5 is beyond"),
    ("sensor_hw of floats", {}, dict(sensor_hw=(4.0, 5)), "EINVAL", r"sensor_hw = 4.0 is not a whole number"),
    ("dt_us negative", {}, dict(dt_us=-1), "EINVAL", r"dt_us = -1 must be in \[0, 2\^31\)"),
    ("dt_us 2^31", {}, dict(dt_us=1 << 31), "EINVAL", r"dt_us = 2147483648 must be in"),
    ("dt_us a float", {}, dict(dt_us=1000.0), "EINVAL", r"dt_us = 1000.0 is not a whole number"),
    ("radius 0", {}, dict(radius=0), "EINVAL", r"radius = 0; 1 or 2 expected"),
    ("radius 3", {}, dict(radius=3), "EINVAL", r"radius = 3; 1 or 2 expected"),
    ("radius a bool", {}, dict(radius=True), "EINVAL", r"radius = True is not a whole number"),
    ("min_support 0", {}, dict(min_support=0), "EINVAL", r"min_support = 0 must be in \[1, 9\]"),
    ("min_support 10 at radius 1", {}, dict(min_support=10), "EINVAL", r"min_support = 10 must be in \[1, 9\]"),
    ("min_support 26 at radius 2", {}, dict(radius=2, min_support=26), "EINVAL", r"min_support = 26 must be in \[1, 25\]"),
    ("same_polarity a number", {}, dict(same_polarity=1), "EINVAL", r"same_polarity = 1 is neither True nor False"),
    ("include_self a word", {}, dict(include_self="yes"), "EINVAL", r"include_self = 'yes' is neither True nor False"),
    ("bounds of floats", {}, dict(bounds=np.array([0.0, 3.0])), "ESHAPE", r"bounds must be whole numbers in one dimension"),
    ("bounds two-dimensional", {}, dict(bounds=np.zeros((2, 2), np.int64)), "ESHAPE", r"bounds must be whole numbers in one dimension"),
    ("bounds that decrease", {}, dict(bounds=[0, 2, 1, 3]), "EINVAL", r"bounds must not decrease and lie in \[0, 3\]"),
    ("bounds beyond N", {}, dict(bounds=[0, 4]), "EINVAL", r"bounds must not decrease and lie in \[0, 3\]"),
    ("bounds below 0", {}, dict(bounds=[-1, 3]), "EINVAL", r"bounds must not decrease and lie in \[0, 3\]"),
    ("last of another shape", {}, dict(last="int64 [1, 4, 6]"), "ESHAPE", r"last must be a contiguous int64 tensor \[1\]\[4\]\[5\]"),
    ("last without its channel axis", {}, dict(last="int64 [4, 5]"), "ESHAPE", r"last must be a contiguous int64 tensor \[1\]\[4\]\[5\]"),
    ("last of another dtype", {}, dict(last="int32 [1, 4, 5]"), "ESHAPE", r"last must be a contiguous int64 tensor"),
    ("last of one plane with same_polarity", {}, dict(last="int64 [1, 4, 5]", same_polarity=True), "ESHAPE",
     r"last must be a contiguous int64 tensor \[2\]\[4\]\[5\] \(2 planes with same_polarity=True"),
    ("last of two planes without", {}, dict(last="int64 [2, 4, 5]"), "ESHAPE", r"\[1\]\[4\]\[5\] \(1 plane with same_polarity=False"),
    ("last an array", {}, dict(last=np.zeros((1, 4, 5), np.int64)), "ESHAPE", r"last must be a contiguous int64 tensor"),
]


def _tensor(spec):
    import torch
    if not isinstance(spec, str):
        return spec
    dtype, shape = spec.split(" ", 1)
    return torch.zeros([int(v) for v in shape.strip("[]").split(",")], dtype=getattr(torch, dtype))


@pytest.mark.parametrize("what,pos,kw,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_python_layer_refusal(nsof_lib, what, pos, kw, status, message):
    """Each refusal names its argument and comes before any device work: the stream is of CPU tensors, so a call that got past
    its check would raise the 'must be CUDA tensors' error instead, which no pattern here matches."""
    from nsof import _lib
    from nsof.errors import NsofValueError
    ev = _good()
    for i, v in pos.items():
        ev[i] = _tensor(v)
    kw = dict(dict(sensor_hw=(4, 5), dt_us=10), **kw)
    if "last" in kw:
        kw["last"] = _tensor(kw["last"])
    sensor_hw, dt_us = kw.pop("sensor_hw"), kw.pop("dt_us")
    assert "CUDA" not in message
    with pytest.raises(NsofValueError, match=message) as e:
        nsof_lib.events_denoise_dev(*ev, sensor_hw, dt_us, **kw)
    assert e.value.status == getattr(_lib, "NSOF_" + status), what


def test_python_layer_accepts_the_good_arguments_up_to_the_device_check(nsof_lib):
    import torch
    from nsof import _lib
    from nsof.errors import NsofValueError
    for kw in (dict(), dict(dt_us=0), dict(dt_us=(1 << 31) - 1, radius=2, min_support=25), dict(min_support=9, include_self=True),
               dict(same_polarity=True, last=torch.zeros((2, 4, 5), dtype=torch.int64)), dict(last=torch.zeros((1, 4, 5), dtype=torch.int64)),
               dict(bounds=[0, 0, 3, 3]), dict(bounds=np.array([], np.int64)), dict(bounds=np.array([1, 2], np.uint8)),
               dict(sensor_hw=(32767, 32767)), dict(dt_us=np.int64(5), radius=np.int32(2))):
        kw = dict(dict(sensor_hw=(4, 5), dt_us=10), **kw)
        sensor_hw, dt_us = kw.pop("sensor_hw"), kw.pop("dt_us")
        with pytest.raises(NsofValueError, match=r"x, y, p, t \(and last\) must be CUDA tensors on one device") as e:
            nsof_lib.events_denoise_dev(*_good(), sensor_hw, dt_us, **kw)
        assert e.value.status == _lib.NSOF_EINVAL
    with pytest.raises(NsofValueError, match=r"must be CUDA tensors"):   # an empty stream is checked like any other
        nsof_lib.events_denoise_dev(*_good(0), (4, 5), 10)


REFUSED_DICTS = [
    ("not a dict", 1000, r"denoise = 1000; a dict of dt_us and any of radius, min_support, same_polarity, include_self, last"),
    ("without dt_us", dict(radius=2), r"denoise = \{'radius': 2\}; a dict of dt_us"),
    ("an unknown key", dict(dt_us=1000, support=2), r"denoise = .*'support': 2.*a dict of dt_us"),
    ("bounds are the pipeline's", dict(dt_us=1000, bounds=[0]), r"denoise = .*'bounds'.*a dict of dt_us and any of"),
    ("ctx is the pipeline's", dict(dt_us=1000, ctx=None), r"denoise = .*'ctx'.*a dict of dt_us and any of"),
]


@pytest.mark.parametrize("what,denoise,message", REFUSED_DICTS, ids=[r[0] for r in REFUSED_DICTS])
def test_pipeline_refuses_a_bad_denoise_dict(nsof_lib, what, denoise, message):
    import torch
    from nsof import _lib, pipeline
    from nsof.errors import NsofValueError
    frames = torch.zeros((3, 4, 5), dtype=torch.uint8)   # a CPU tensor: past the check, the generator's device refusal
    with pytest.raises(NsofValueError, match=r"video_to_flow_sequence: " + message) as e:
        pipeline.video_to_flow_sequence(frames, frame_us=10, denoise=denoise)
    assert e.value.status == _lib.NSOF_EINVAL, what


REFUSED_VALUES = [
    ("radius 3", dict(dt_us=1000, radius=3), "EINVAL", r"denoise: radius = 3; 1 or 2 expected"),
    ("dt_us 2^31", dict(dt_us=1 << 31), "EINVAL", r"denoise: dt_us = 2147483648 must be in"),
    ("dt_us a float", dict(dt_us=5.0), "EINVAL", r"denoise: dt_us = 5.0 is not a whole number"),
    ("min_support 10", dict(dt_us=5, min_support=10), "EINVAL", r"denoise: min_support = 10 must be in \[1, 9\]"),
    ("same_polarity a number", dict(dt_us=5, same_polarity=1), "EINVAL", r"denoise: same_polarity = 1 is neither True nor False"),
    ("last of another shape", dict(dt_us=5, last="int64 [1, 4, 6]"), "ESHAPE", r"denoise: last must be a contiguous int64 tensor \[1\]\[4\]\[5\]"),
    ("last of one plane with same_polarity", dict(dt_us=5, same_polarity=True, last="int64 [1, 4, 5]"), "ESHAPE",
     r"denoise: last must be a contiguous int64 tensor \[2\]\[4\]\[5\]"),
]


@pytest.mark.parametrize("what,denoise,status,message", REFUSED_VALUES, ids=[r[0] for r in REFUSED_VALUES])
def test_pipeline_refuses_a_bad_value_before_the_generator_runs(nsof_lib, what, denoise, status, message):
    """The frames are a CPU tensor: had the generator been reached, its 'must be CUDA tensors' refusal would come instead."""
    import torch
    from nsof import _lib, pipeline
    from nsof.errors import NsofValueError
    frames = torch.zeros((3, 4, 5), dtype=torch.uint8)
    denoise = dict(denoise)
    if "last" in denoise:
        denoise["last"] = _tensor(denoise["last"])
    with pytest.raises(NsofValueError, match=r"video_to_flow_sequence: " + message) as e:
        pipeline.video_to_flow_sequence(frames, frame_us=10, denoise=denoise)
    assert e.value.status == getattr(_lib, "NSOF_" + status), what


def test_pipeline_takes_a_good_denoise_dict_up_to_the_device_check(nsof_lib):
    import torch
    from nsof import pipeline
    from nsof.errors import NsofValueError
    frames = torch.zeros((3, 4, 5), dtype=torch.uint8)
    for denoise in (None, dict(dt_us=1000), dict(dt_us=5, radius=2, min_support=3, same_polarity=True, include_self=True, last=None)):
        with pytest.raises(NsofValueError, match=r"events_from_frames_dev: frames \(and ref\) must be CUDA tensors"):
            pipeline.video_to_flow_sequence(frames, frame_us=10, denoise=denoise)


def test_new_symbols_are_declared_exported_and_bound(nsof_lib):
    from nsof import _lib, denoise
    header = open(os.path.join(ROOT, "include", "nsof.h")).read()
    assert re.search(r"#define NSOF_ABI_VERSION 3\b", header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name, n_args in ARGS.items():
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.nsof_abi_version() == 3 and _lib.K_COUNT == 11   # new entries only
    assert nsof_lib.events_denoise_dev is denoise.events_denoise_dev and denoise.NEVER == NEVER


def test_the_c_entries_refuse_before_they_need_a_device(nsof_lib):
    """A null context is refused first of all (NSOF_EINVAL), so no device is touched."""
    from nsof import _lib
    lib = _lib.load()
    assert lib.nsof_events_denoise_mark_dev(None, None, None, None, None, 0, 4, 5, 10, 1, 1, 0, 0, None, None, 0, None, None, None) == _lib.NSOF_EINVAL
    assert lib.nsof_events_denoise_compact_dev(None, None, None, None, None, 0, 4, 5, 0, None, None, 0, None, None, None, None, None) == _lib.NSOF_EINVAL
