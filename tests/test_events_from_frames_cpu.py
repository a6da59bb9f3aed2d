"""CPU: the level-crossing event generator's model (tests/events_from_frames_ref.py) against the data the reference's
generator produced, its chunking and ordering properties, and the Python layer's refusals (no device needed)."""
import numpy as np
import pytest

from conftest import golden_path
from events_from_frames_ref import events_from_frames_ref, units

SETTINGS = {"default": {}, "small": dict(H=60, W=90, box_h=20, box_w=11, speed_pps=700, duration_s=0.2)}


@pytest.fixture(scope="module")
def random_frames():
    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (6, 13, 17), dtype=np.uint8)
    frames[3] = frames[2]   # an empty pair
    return frames, np.array([0, 1000, 1700, 2100, 5000, 5004], np.int64)


@pytest.mark.parametrize("name", list(SETTINGS))
def test_box_frames_give_the_reference_generators_events(nsof_lib, name):
    """render_box_frames + the model in "frame" mode with a threshold of one level == the arrays the reference produced."""
    g = np.load(golden_path("synth_events.npz"))
    frames, times = nsof_lib.render_box_frames(**SETTINGS[name])
    assert frames.dtype == np.uint8 and times.dtype == np.int64 and len(frames) == len(times)
    for thr in (1.0, 0.51):   # any threshold in (1/2, 1] grey levels: one crossing per unit step
        ev = events_from_frames_ref(frames, times, units(thr), units(thr), timestamps="frame")
        for key in "xypt":
            assert np.array_equal(ev[key], g[f"{name}_{key}"]), (name, thr, key)
        if name == "default":
            break   # one pass over the 3000 frames is enough


def test_box_leaving_the_sensor_matches_the_host_generator(nsof_lib):
    kw = dict(H=40, W=64, box_h=50, box_w=9, speed_pps=900, duration_s=0.1)   # taller than the sensor, and it leaves it
    frames, times = nsof_lib.render_box_frames(**kw)
    assert frames[-1].sum() == 0 and frames.any()
    x, y, p, t = nsof_lib.generate_synthetic_events(**kw)
    ev = events_from_frames_ref(frames, times, units(1), units(1), timestamps="frame")
    for got, want in ((ev["x"], x), (ev["y"], y), (ev["p"], p), (ev["t"], t)):
        assert len(want) and np.array_equal(got, want)


@pytest.mark.parametrize("timestamps", ["frame", "linear"])
def test_chunked_equals_one_shot_and_t_never_decreases(random_frames, timestamps):
    frames, times = random_frames
    seen = []
    one = events_from_frames_ref(frames, times, units(7), units(20), timestamps=timestamps, on_frame=lambda k, r, b: seen.append(k))
    assert seen == list(range(len(frames)))   # the invariant on r was asserted after each of them
    assert len(one["t"]) > 100 and (np.diff(one["t"]) >= 0).all()
    assert one["frame_bounds"][3] == one["frame_bounds"][4]   # the unchanged frame emits nothing
    for k in range(len(frames)):
        a = events_from_frames_ref(frames[:k + 1], times[:k + 1], units(7), units(20), timestamps=timestamps)
        b = events_from_frames_ref(frames[k:], times[k:], units(7), units(20), ref=a["ref"], timestamps=timestamps)
        assert b["frame_bounds"][1] == 0   # the repeated frame emits nothing
        for key in "xypt":
            assert np.array_equal(np.concatenate([a[key], b[key]]), one[key]), (k, key)
        assert np.array_equal(np.concatenate([a["frame_bounds"], a["frame_bounds"][-1] + b["frame_bounds"][2:]]), one["frame_bounds"])
        assert np.array_equal(b["ref"], one["ref"])


def test_linear_stamps_lie_inside_their_pair(random_frames):
    frames, times = random_frames
    ev = events_from_frames_ref(frames, times, units(3), units(3), timestamps="linear")
    fb = ev["frame_bounds"]
    assert (ev["t"][:fb[1]] == times[0]).all()
    for k in range(1, len(frames)):
        t = ev["t"][fb[k]:fb[k + 1]]
        assert ((t >= times[k - 1]) & (t <= times[k])).all() and (np.diff(t) >= 0).all()


def _good():
    import torch
    return torch.zeros((3, 4, 5), dtype=torch.uint8)


# what is wrong, the frames (None: the good CPU stack), the arguments, the status, what the message must name
REFUSALS = [
    ("dtype", lambda g: g.float(), dict(frame_us=10), "EINVAL", r"frames must be a uint8 tensor"),
    ("dimensions", lambda g: g[0], dict(frame_us=10), "ESHAPE", r"frames must be \[n\]\[H\]\[W\] with dense rows"),
    ("rows not dense", lambda g: g.permute(0, 2, 1), dict(frame_us=10), "ESHAPE", r"with dense rows"),
    ("times do not increase", None, dict(times_us=[0, 5, 5]), "EINVAL", r"times_us\[2\] = 5 after 5: the times must increase strictly"),
    ("times decrease", None, dict(times_us=[0, 5, 4]), "EINVAL", r"times_us\[2\] = 4 after 5"),
    ("a gap of 2^31", None, dict(times_us=[0, 5, 5 + (1 << 31)]), "EINVAL", r"times_us\[2\] = 2147483653 after 5.*less than 2\^31"),
    ("one time per frame", None, dict(times_us=[0, 5]), "ESHAPE", r"times_us must be 3 whole numbers"),
    ("fractional times", None, dict(times_us=[0.0, 5.0, 9.5]), "ESHAPE", r"times_us must be 3 whole numbers"),
    ("both times_us and frame_us", None, dict(times_us=[0, 5, 9], frame_us=10), "EINVAL", r"either times_us or frame_us, not both"),
    ("neither times_us nor frame_us", None, dict(), "EINVAL", r"give either times_us or frame_us$"),
    ("frame_us 0", None, dict(frame_us=0), "EINVAL", r"frame_us = 0 must be in \[1, 2\^31\)"),
    ("frame_us 2^31", None, dict(frame_us=1 << 31), "EINVAL", r"frame_us = 2147483648 must be in"),
    ("frame_us a float", None, dict(frame_us=10.0), "EINVAL", r"frame_us = 10.0 is not a whole number"),
    ("threshold rounds to 0", None, dict(frame_us=10, threshold=0.001), "EINVAL", r"threshold = 0.001 grey levels is 0 table units"),
    ("threshold_off 0", None, dict(frame_us=10, threshold_off=0.0), "EINVAL", r"threshold_off = 0.0 grey levels is 0 table units"),
    ("threshold negative", None, dict(frame_us=10, threshold=-3), "EINVAL", r"threshold = -3 grey levels is -768 table units"),
    ("threshold NaN", None, dict(frame_us=10, threshold=float("nan")), "EINVAL", r"threshold = nan is not a finite number"),
    ("timestamps", None, dict(frame_us=10, timestamps="exact"), "EINVAL", r"timestamps = 'exact'"),
    ("ref a word", None, dict(frame_us=10, ref="last"), "EINVAL", r"ref = 'last'"),
    ("ref of another size", None, dict(frame_us=10, ref="int32 [4][6]"), "ESHAPE", r"ref must be a contiguous int32 tensor \[4\]\[5\]"),
    ("ref of another dtype", None, dict(frame_us=10, ref="int64 [4][5]"), "ESHAPE", r"ref must be a contiguous int32 tensor"),
    ("p_off beyond int8", None, dict(frame_us=10, p_off=-200), "EINVAL", r"p_off = -200 does not fit an int8"),
    ("p_on beyond int8", None, dict(frame_us=10, p_on=128), "EINVAL", r"p_on = 128 does not fit an int8"),
    ("response above 2^30", None, dict(frame_us=10, response=np.arange(256) * (1 << 23)), "EINVAL", r"response entries must lie in \[0, 2\^30\]"),
    ("response negative", None, dict(frame_us=10, response=np.arange(256) - 1), "EINVAL", r"response entries must lie in \[0, 2\^30\] \(got -1"),
    ("response of 255 entries", None, dict(frame_us=10, response=np.arange(255)), "ESHAPE", r"response must be 256 whole numbers"),
    ("a plane holding a 0", None, dict(frame_us=10, threshold_maps=np.zeros((4, 5, 2))), "EINVAL",
     r"threshold_maps\[0\]\[0\]\[0\] = .*0 table units"),
    ("a plane with one 0", None, dict(frame_us=10, threshold_maps="one zero"), "EINVAL", r"threshold_maps\[2\]\[3\]\[1\] = "),
    ("a plane of another shape", None, dict(frame_us=10, threshold_maps=np.ones((4, 5))), "ESHAPE", r"threshold_maps must be numbers \[4\]\[5\]\[2\]"),
]


@pytest.mark.parametrize("what,frames,kw,status,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_python_layer_refusal(nsof_lib, what, frames, kw, status, message):
    """Each refusal names its argument and comes before any device work (the stack is a CPU tensor, so a call that got
    past its check would raise the 'must be CUDA tensors' error instead, which no pattern here matches)."""
    import torch
    from nsof import _lib
    from nsof.errors import NsofValueError
    g = _good()
    kw = dict(kw)
    if isinstance(kw.get("ref"), str) and kw["ref"].startswith("int"):
        kw["ref"] = torch.zeros((4, 6) if "[6]" in kw["ref"] else (4, 5), dtype=getattr(torch, kw["ref"].split()[0]))
    if isinstance(kw.get("threshold_maps"), str):
        kw["threshold_maps"] = np.full((4, 5, 2), 2.0)
        kw["threshold_maps"][2, 3, 1] = 0.0
    assert "CUDA" not in message
    with pytest.raises(NsofValueError, match=message) as e:
        nsof_lib.events_from_frames_dev(g if frames is None else frames(g), **kw)
    assert e.value.status == getattr(_lib, "NSOF_" + status), what


def test_python_layer_accepts_the_good_arguments_up_to_the_device_check(nsof_lib):
    """The arguments the refusal cases vary are fine here, in every accepted form: only the missing device is refused."""
    import torch
    from nsof import _lib, pipeline
    from nsof.errors import NsofValueError
    g = _good()
    for kw in (dict(frame_us=10), dict(times_us=[0, 5, 5 + (1 << 31) - 1]), dict(times_us=np.array([3, 4, 9], np.uint32)),
               dict(frame_us=(1 << 31) - 1, threshold=1 / 256, threshold_off=0.002, timestamps="frame", ref="first", p_on=127, p_off=-128),
               dict(frame_us=10, response=np.full(256, 1 << 30), threshold_maps=np.full((4, 5, 2), 1 / 256)),
               dict(frame_us=10, ref=torch.zeros((4, 5), dtype=torch.int32))):
        with pytest.raises(NsofValueError, match=r"frames \(and ref\) must be CUDA tensors on one device") as e:
            nsof_lib.events_from_frames_dev(g, **kw)
        assert e.value.status == _lib.NSOF_EINVAL
    bgr = torch.zeros((3, 4, 5, 3), dtype=torch.uint8)
    with pytest.raises(NsofValueError, match=r"events_from_video_dev: frames must be a CUDA tensor"):
        nsof_lib.events_from_video_dev(bgr, frame_us=10)
    with pytest.raises(NsofValueError, match=r"frames must be a uint8 tensor \[n\]\[H\]\[W\]\[3\]"):
        nsof_lib.events_from_video_dev(g, frame_us=10)
    with pytest.raises(NsofValueError, match=r"code must be RGB2GRAY or BGR2GRAY"):
        nsof_lib.events_from_video_dev(bgr, frame_us=10, code="GRAY")
    assert pipeline.events_from_frames_dev is nsof_lib.events_from_frames_dev and callable(pipeline.video_to_flow_sequence)


