"""CPU: the event generator's sensor model (tests/events_sensor_ref.py) -- its defaults against the plain model, chunking at
every cut, the refractory spacing, the noise generator's words and counts -- and, without a device, the Python layer's
refusals and the new symbols."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from events_from_frames_ref import drifting_texture, events_from_frames_ref, units
from events_sensor_ref import NEVER, events_sensor_ref, noise_candidates, noise_words, rate_q

TIMES = np.array([0, 33333, 50000, 120000, 121000, 200000, 233333], np.int64)   # uneven
ARGS = {"nsof_events_from_frames_sensor_count_dev": 17, "nsof_events_from_frames_sensor_emit_dev": 26, "nsof_events_noise_draw": 4}


@pytest.fixture(scope="module")
def texture():
    return drifting_texture(7, 19, 37)


def _same(a, b, keys=("x", "y", "p", "t", "frame_bounds", "ref")):
    for k in keys:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
@pytest.mark.parametrize("ref", [None, "first"])
def test_defaults_equal_the_plain_model(texture, timestamps, ref):
    one = events_sensor_ref(texture, TIMES, units(10), units(7), ref=ref, timestamps=timestamps)
    want = events_from_frames_ref(texture, TIMES, units(10), units(7), ref=ref, timestamps=timestamps)
    assert len(want["x"]) > 1000 and not one["noise"].any()
    _same(one, want)
    fired = np.zeros((19, 37), bool)
    fired[want["y"], want["x"]] = True
    assert ((one["t_ok"] == NEVER) == ~fired).all()   # t_ok of a pixel: its last event, or never


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
@pytest.mark.parametrize("refractory_us,hz", [(0, 5), (1, 5), (11111, 2), (70000, 5), (70000, 0)])
def test_chunked_equals_one_shot_at_every_cut(texture, timestamps, refractory_us, hz):
    kw = dict(timestamps=timestamps, refractory_us=refractory_us, seed=77, rate_on=rate_q(hz), rate_off=rate_q(hz))
    one = events_sensor_ref(texture, TIMES, units(10), units(10), ref="first", first_frame=40, **kw)
    if hz:
        assert one["noise"].min() > 100
    for k in range(7):
        a = events_sensor_ref(texture[:k + 1], TIMES[:k + 1], units(10), units(10), ref="first", first_frame=40, **kw)
        b = events_sensor_ref(texture[k:], TIMES[k:], units(10), units(10), ref=a["ref"], t_ok=a["t_ok"], first_frame=40 + k, **kw)
        assert b["frame_bounds"][1] == 0   # the repeated frame emits nothing
        for key in "xypt":
            assert np.array_equal(np.concatenate([a[key], b[key]]), one[key]), (k, key)
        assert np.array_equal(np.concatenate([a["frame_bounds"], a["frame_bounds"][-1] + b["frame_bounds"][2:]]), one["frame_bounds"])
        assert np.array_equal(b["ref"], one["ref"]) and np.array_equal(b["t_ok"], one["t_ok"])


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
@pytest.mark.parametrize("refractory_us", [1, 11111, 70000])
def test_events_of_a_pixel_are_a_refractory_time_apart(texture, timestamps, refractory_us):
    ev = events_sensor_ref(texture, TIMES, units(4), units(4), timestamps=timestamps, refractory_us=refractory_us, seed=3,
                           rate_on=rate_q(5), rate_off=rate_q(5))
    plain = events_from_frames_ref(texture, TIMES, units(4), units(4), timestamps=timestamps)
    assert np.array_equal(ev["ref"], plain["ref"])   # the comparator resets whether or not the read-out is blocked
    assert 0 < len(ev["x"]) < len(plain["x"]) and (np.diff(ev["t"]) >= 0).all()
    pix = ev["y"].astype(np.int64) * 37 + ev["x"]
    order = np.argsort(pix, kind="stable")   # the stream is in time order, so each pixel's events stay in it
    same_pixel = np.diff(pix[order]) == 0
    gaps = np.diff(ev["t"][order])[same_pixel]
    assert same_pixel.sum() > 100 and gaps.min() >= refractory_us
    last = np.full(19 * 37, NEVER, np.int64)
    last[pix] = ev["t"] + refractory_us   # later events overwrite earlier ones
    assert np.array_equal(last.reshape(19, 37), ev["t_ok"])


def test_philox_known_answer_and_the_librarys_draw(nsof_lib):
    from accum_c2c_ref import philox4x32_10
    assert [int(v) for v in philox4x32_10(0, 0, 0, 0, 0, 0)] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    rng = np.random.default_rng(1)
    cases = [(0, 0, 0), (2**64 - 1, 2**32 - 1, 2**62), (5, 702, 63)] + \
            [(int(rng.integers(0, 2**63)) * 2 + 1, int(rng.integers(0, 2**32)), int(rng.integers(0, 2**62))) for _ in range(20)]
    for seed, pixel, frame in cases:
        got = nsof_lib.events_noise_draw(seed, pixel, frame)
        assert got.dtype == np.uint32 and got.shape == (4,)
        assert [int(v) for v in got] == [int(v) for v in noise_words(seed, pixel, frame)], (seed, pixel, frame)
    # the fourth counter word keeps the block apart from a c2c draw of the same (seed, pixel, slice)
    assert [int(v) for v in nsof_lib.events_noise_draw(9, 4, 6)] != [int(v) for v in philox4x32_10(4, 6, 0, 0, 9, 0)]
    from nsof.errors import NsofValueError
    for bad in ((-1, 0, 0), (2**64, 0, 0), (0, 2**32, 0), (0, 0, -1), (0, 0, 2**62 + 1), (0.5, 0, 0), (0, True, 0)):
        with pytest.raises(NsofValueError, match="events_noise_draw"):
            nsof_lib.events_noise_draw(*bad)


@pytest.mark.parametrize("hz", [0.1, 1, 10])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_noise_counts_lie_within_four_standard_deviations(seed, hz):
    """703 pixels x 64 intervals of 33333 us: a condition on fixed draws (the worst of the 24 is 2.72 standard deviations)."""
    q, delta, npx, n = rate_q(hz), 33333, 703, 64
    rate = np.full(npx, q, np.uint64)
    count = np.zeros(2, np.int64)
    for f in range(1, n + 1):
        has_on, o_on, has_off, o_off = noise_candidates(seed, npx, f, delta, rate, rate)
        count += (has_on.sum(), has_off.sum())
        assert o_on.min() >= 0 and o_on.max() < delta and o_off.min() >= 0 and o_off.max() < delta
    p = q * delta / 2.0**32
    mean, sd = npx * n * p, np.sqrt(npx * n * p * (1 - p))
    for pol in (0, 1):
        assert abs(count[pol] - mean) <= 4 * sd, (pol, count[pol], mean, sd)


def _good():
    import torch
    return torch.zeros((3, 4, 5), dtype=torch.uint8)


# what is wrong, the arguments, the status, what the message must name
REFUSALS = [
    ("refractory negative", dict(refractory_us=-1), "EINVAL", r"refractory_us = -1 must be in \[0, 2\^31\)"),
    ("refractory 2^31", dict(refractory_us=1 << 31), "EINVAL", r"refractory_us = 2147483648 must be in"),
    ("refractory a float", dict(refractory_us=800.0), "EINVAL", r"refractory_us = 800.0 is not a whole number"),
    ("first_frame negative", dict(first_frame=-1), "EINVAL", r"first_frame = -1 with 3 frames"),
    ("first_frame beyond 2^62", dict(first_frame=(1 << 62) - 2), "EINVAL", r"first_frame = 4611686018427387902 with 3 frames"),
    ("first_frame a float", dict(first_frame=1.0), "EINVAL", r"first_frame = 1.0 is not a whole number"),
    ("noise not a dict", dict(noise=5.0), "EINVAL", r"noise = 5.0; a dict with 'seed'"),
    ("noise without a seed", dict(noise=dict(rate_hz=1)), "EINVAL", r"a dict with 'seed'"),
    ("noise with an unknown key", dict(noise=dict(seed=1, rate=1)), "EINVAL", r"a dict with 'seed'"),
    ("seed negative", dict(noise=dict(seed=-1, rate_hz=1)), "EINVAL", r"noise\['seed'\] = -1 is not a whole number in \[0, 2\^64\)"),
    ("seed 2^64", dict(noise=dict(seed=1 << 64, rate_hz=1)), "EINVAL", r"noise\['seed'\] = 18446744073709551616"),
    ("seed a float", dict(noise=dict(seed=1.5, rate_hz=1)), "EINVAL", r"noise\['seed'\] = 1.5"),
    ("no rates", dict(noise=dict(seed=1)), "EINVAL", r"gives its rates 0 ways \(none\)"),
    ("rates two ways", dict(noise=dict(seed=1, rate_hz=1, rate_on_hz=2)), "EINVAL", r"gives its rates 2 ways \(rate_hz, rate_on_hz / rate_off_hz\)"),
    ("rate and maps", dict(noise=dict(seed=1, rate_hz=1, rate_maps=np.zeros((4, 5, 2)))), "EINVAL", r"gives its rates 2 ways \(rate_hz, rate_maps\)"),
    ("rate negative", dict(noise=dict(seed=1, rate_hz=-0.5)), "EINVAL", r"noise\['rate_hz'\] = -0.5 Hz is -2147 units"),
    ("rate of 1 MHz", dict(noise=dict(seed=1, rate_on_hz=1e6)), "EINVAL", r"noise\['rate_on_hz'\] = 1000000.0 Hz is 4294967296 units"),
    ("rate NaN", dict(noise=dict(seed=1, rate_off_hz=float("nan"))), "EINVAL", r"noise\['rate_off_hz'\] = nan is not a finite number"),
    ("rate a word", dict(noise=dict(seed=1, rate_hz="1")), "EINVAL", r"noise\['rate_hz'\] = '1' is not a finite number"),
    ("maps of another shape", dict(noise=dict(seed=1, rate_maps=np.zeros((4, 5)))), "ESHAPE", r"noise\['rate_maps'\] must be numbers \[4\]\[5\]\[2\]"),
    ("maps with a negative rate", dict(noise=dict(seed=1, rate_maps="one negative")), "EINVAL", r"noise\['rate_maps'\]\[2\]\[3\]\[1\] = -1.0 Hz"),
    ("maps with an infinite rate", dict(noise=dict(seed=1, rate_maps="one infinite")), "EINVAL", r"noise\['rate_maps'\] holds a value that is not finite"),
    ("t_ok of another dtype", dict(t_ok="int32 [4][5]"), "ESHAPE", r"t_ok must be a contiguous int64 tensor \[4\]\[5\]"),
    ("t_ok of another size", dict(t_ok="int64 [4][6]"), "ESHAPE", r"t_ok must be a contiguous int64 tensor \[4\]\[5\]"),
    ("t_ok an array", dict(t_ok=np.zeros((4, 5), np.int64)), "ESHAPE", r"t_ok must be a contiguous int64 tensor"),
]


@pytest.mark.parametrize("what,kw,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_python_layer_refusal(nsof_lib, what, kw, status, message):
    """Each refusal names its argument and comes before any device work: the stack is a CPU tensor, so a call that got past
    its check would raise the 'must be CUDA tensors' error instead, which no pattern here matches."""
    import torch
    from nsof import _lib
    from nsof.errors import NsofValueError
    kw = dict(kw)
    if isinstance(kw.get("t_ok"), str):
        kw["t_ok"] = torch.zeros((4, 6) if "[6]" in kw["t_ok"] else (4, 5), dtype=getattr(torch, kw["t_ok"].split()[0]))
    if isinstance(kw.get("noise"), dict) and isinstance(kw["noise"].get("rate_maps"), str):
        maps = np.full((4, 5, 2), 2.0)
        maps[2, 3, 1] = -1.0 if "negative" in kw["noise"]["rate_maps"] else np.inf
        kw["noise"] = dict(kw["noise"], rate_maps=maps)
    assert "CUDA" not in message
    with pytest.raises(NsofValueError, match=message) as e:
        nsof_lib.events_from_frames_dev(_good(), frame_us=10, **kw)
    assert e.value.status == getattr(_lib, "NSOF_" + status), what


def test_python_layer_accepts_the_good_arguments_up_to_the_device_check(nsof_lib):
    import torch
    from nsof import _lib, pipeline
    from nsof.errors import NsofValueError
    g = _good()
    for kw in (dict(refractory_us=0), dict(refractory_us=(1 << 31) - 1, first_frame=(1 << 62) - 3),
               dict(noise=dict(seed=(1 << 64) - 1, rate_hz=0)), dict(noise=dict(seed=0, rate_on_hz=999999.9)),
               dict(noise=dict(seed=np.int64(4), rate_off_hz=np.float32(2))), dict(noise=dict(seed=1, rate_maps=np.ones((4, 5, 2)))),
               dict(noise=dict(seed=1, rate_maps=torch.ones((4, 5, 2)))), dict(t_ok=torch.zeros((4, 5), dtype=torch.int64))):
        with pytest.raises(NsofValueError, match=r"frames \(and ref\) must be CUDA tensors on one device") as e:
            nsof_lib.events_from_frames_dev(g, frame_us=10, **kw)
        assert e.value.status == _lib.NSOF_EINVAL
    with pytest.raises(NsofValueError, match=r"video_to_flow_sequence: sensor = .*a dict of refractory_us, noise, t_ok, first_frame"):
        pipeline.video_to_flow_sequence(g, frame_us=10, sensor=dict(refractory=5))
    with pytest.raises(NsofValueError, match=r"refractory_us = -2 must be in"):
        pipeline.video_to_flow_sequence(g, frame_us=10, sensor=dict(refractory_us=-2))
    assert rate_q(1) == 4295 and rate_q(0.1) == 429


def test_new_symbols_are_declared_exported_and_bound(nsof_lib):
    from nsof import _lib, events
    header = open(os.path.join(ROOT, "include", "nsof.h")).read()
    assert re.search(r"#define NSOF_ABI_VERSION 3\b", header)
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name, n_args in ARGS.items():
        decl = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", header)
        assert decl, name
        assert len(decl.group(1).split(",")) == n_args, name
        assert len(_lib.SIGNATURES[name][1]) == n_args and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    fields = re.search(r"typedef struct nsof_events_sensor \{(.*?)\} nsof_events_sensor;", header, flags=re.S)
    assert fields and [f.strip().split()[-1].lstrip("*") for f in fields.group(1).replace(",", ";").split(";") if f.strip()] == \
        [f[0] for f in _lib.EventsSensor._fields_]
    assert lib.nsof_abi_version() == 3   # new entries only
    assert nsof_lib.events_noise_draw is events.events_noise_draw
