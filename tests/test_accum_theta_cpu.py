"""CPU: scheme 1's event-count threshold (THETA_EVENTS) -- the yardsticks and the Python layer, no device.

tests/golden/accum_theta_v1.npz was made by running the reference with its module knob THETA_EVENTS set
(tests/golden/gen_accum_theta_golden.py).  tests/accum_theta_ref.py restates the run in NumPy (``accum_params_ref.simulate``
with the count test) and must reproduce it: bit for bit with the silent voltage in the dead zone (only the driven cells
compute anything, and there the restatement's powers agree with NumPy's on this stream), within W_ATOL / R_RTOL -- the
project's bounds for the reference's SIMD pow / exp -- on the leak stream, where every pixel computes every slice.  The
same file holds the stream filter the GPU tests use as their exact yardstick; here it is checked against the restatement."""
import gzip
import inspect
import json

import numpy as np
import pytest

import accum_theta_ref as T
from conftest import golden_path

F = np.float32
W_ATOL = 5e-7       # tests/test_accum_gpu.py
R_RTOL = 2e-6
H, W = 48, 64       # noqa: N816
CASES = [("dead", 2), ("dead", 3), ("dead", 5), ("leak", 2), ("leak", 3)]


@pytest.fixture(scope="module")
def fixture():
    return np.load(golden_path("accum_theta_v1.npz"))


def stream_of(d, name):
    return d[f"{name}_x"], d[f"{name}_y"], d[f"{name}_p"], d[f"{name}_t"]


def test_fixture_is_not_vacuous(fixture):
    """Every case drives some cells and leaves some out: the counts the issue records."""
    want = {"dead": (100, 15214, {2: 2117, 3: 1291, 5: 365}), "leak": (200, 5645, {2: 311, 3: 40})}
    for name, (n_slices, n_cells, reach) in want.items():
        x, y, p, t = stream_of(fixture, name)
        idx = T.R.slice_bounds(t, 1000)
        assert len(idx) - 1 == n_slices
        sl, c = T.cell_counts(x, y, idx, W)
        cells = np.unique(np.stack([sl, y[idx[0]:idx[-1]].astype(np.int64), x[idx[0]:idx[-1]].astype(np.int64), c]), axis=1)
        assert cells.shape[1] == n_cells
        for th, n in reach.items():
            assert int((cells[3] >= th).sum()) == n, (name, th)
        assert [int(v) for v in fixture[f"{name}_thetas"]] == sorted(reach)


@pytest.mark.parametrize("name,theta", CASES)
def test_restatement_reproduces_the_reference(fixture, name, theta):
    x, y, p, t = stream_of(fixture, name)
    got = T.simulate(x, y, t, H, W, 1000, float(fixture[f"{name}_active_v"]), float(fixture[f"{name}_silent_v"]), theta)
    w_ref, r_ref = fixture[f"{name}_th{theta}_w_final"], fixture[f"{name}_th{theta}_resistances"]
    assert got["resistances"].shape[0] == int(fixture[f"{name}_n_snapshots"])
    rr = got["resistances"][fixture["snap_idx"]]
    if name == "dead":
        assert np.array_equal(got["w_final"].view(np.int32), w_ref.view(np.int32))
        # the resistance map goes through the reference's float32 exp on every pixel: the project's bound for it
        assert (np.abs(rr - r_ref) / r_ref).max() <= R_RTOL
    else:
        assert np.abs(got["w_final"] - w_ref).max() <= W_ATOL
        assert (np.abs(rr - r_ref) / r_ref).max() <= R_RTOL
    # a threshold changes the result: the fixture differs from the threshold-1 run
    one = T.simulate(x, y, t, H, W, 1000, float(fixture[f"{name}_active_v"]), float(fixture[f"{name}_silent_v"]), 1)
    assert np.abs(one["w_final"] - w_ref).max() > 1e-3


@pytest.mark.parametrize("name,theta", CASES)
def test_threshold_run_is_the_filtered_stream_at_threshold_one(fixture, name, theta):
    """The definition the GPU tests rest on, checked on the restatement: bit for bit."""
    x, y, p, t = stream_of(fixture, name)
    idx = T.R.slice_bounds(t, 1000)
    (xf, yf, pf, tf), bf = T.filter_stream(x, y, p, t, idx, theta, W)
    assert 0 < xf.size < x.size and bf[-1] == xf.size and len(bf) == len(idx)
    av, sv = float(fixture[f"{name}_active_v"]), float(fixture[f"{name}_silent_v"])
    # the filtered stream keeps its slice grid only through explicit bounds: walk them here as simulate walks its own
    m = T.R.f32_model()
    w = np.full((H, W), m["wini"], F)
    for s in range(len(bf) - 1):
        V = np.full((H, W), F(sv), F)  # noqa: N806
        V[yf[bf[s]:bf[s + 1]], xf[bf[s]:bf[s + 1]]] = F(av)
        w = T.R.update_state(w, V, m)
    want = T.simulate(x, y, t, H, W, 1000, av, sv, theta)["w_final"]
    assert np.array_equal(w.view(np.int32), want.view(np.int32))


def test_filter_keeps_slices_and_polarity_plays_no_part():
    x = np.int16([3, 3, 4, 3, 5, 5, 5, 9])
    y = np.int16([1, 1, 1, 1, 2, 2, 2, 0])
    p = np.int8([0, 1, 1, -1, 0, 0, 1, 1])
    t = np.int64([0, 10, 20, 1500, 3000, 3001, 3002, 3003])
    bounds = np.int64([0, 3, 4, 4, 8])            # slice 2 is empty
    (xf, yf, pf, tf), bf = T.filter_stream(x, y, p, t, bounds, 2, 16)
    assert xf.tolist() == [3, 3, 5, 5, 5] and pf.tolist() == [0, 1, 0, 0, 1] and bf.tolist() == [0, 2, 2, 2, 5]
    (xf, _, _, _), bf = T.filter_stream(x, y, p, t, bounds, 3, 16)
    assert xf.tolist() == [5, 5, 5] and bf.tolist() == [0, 0, 0, 0, 3]
    (xf, _, _, _), bf = T.filter_stream(x, y, p, t, bounds, 1, 16)
    assert xf.tolist() == x.tolist() and bf.tolist() == bounds.tolist()


# ---- the Python layer without a device -------------------------------------------------------------------------------
class _Read(Exception):
    pass


class _Events:
    """An event tuple that says when it is read."""

    def __iter__(self):
        raise _Read


@pytest.mark.parametrize("bad", [0, -1, 1.5, "2", True, [2], 2**31])
def test_simulate_refuses_a_bad_threshold_before_the_events_are_read(nsof_lib, bad):
    with pytest.raises(nsof_lib.error) as e:
        nsof_lib.simulate(_Events(), version=1, theta_events=bad)
    assert "theta_events" in str(e.value)
    with pytest.raises(_Read):   # a good one gets as far as the events
        nsof_lib.simulate(_Events(), version=1, theta_events=2)


def test_scheme_two_has_no_threshold(nsof_lib):
    with pytest.raises(nsof_lib.error) as e:
        nsof_lib.simulate(_Events(), version=2, theta_events=2)
    assert "scheme 2" in str(e.value)
    with pytest.raises(_Read):
        nsof_lib.simulate(_Events(), version=2, theta_events=1)
    with pytest.raises(_Read):
        nsof_lib.simulate(_Events(), version=2)
    from nsof import accumulator as A  # noqa: N812
    with pytest.raises(nsof_lib.error):   # the accumulator refuses before it creates anything (no context is touched)
        A.Accumulator(4, 4, 2, theta_events=2, ctx=object())
    with pytest.raises(nsof_lib.error):
        A.Accumulator(4, 4, 1, theta_events=0, ctx=object())


def test_metadata_records_the_threshold_used(nsof_lib, tmp_path):
    from nsof import accumulator as A  # noqa: N812
    out = dict(w_final=np.zeros((2, 2), F), resistances=np.ones((1, 2, 2), F), w_final_b=np.zeros((2, 2), F),
               resistances_b=np.ones((1, 2, 2), F))

    def meta(prefix, version):
        with gzip.open(prefix.with_suffix(f".V{version}.json.gz"), "rt") as fp:
            return json.load(fp)
    A._save_outputs(tmp_path / "a.x", out, 1, 1000, "split", None, theta_events=5)
    assert meta(tmp_path / "a.x", 1)["theta_events"] == 5
    A._save_outputs(tmp_path / "b.x", out, 1, 1000, "split", None)
    assert meta(tmp_path / "b.x", 1)["theta_events"] == A.THETA_EVENTS == 1
    A._save_outputs(tmp_path / "c.x", out, 2, 1000, "split", None, theta_events=1)
    assert meta(tmp_path / "c.x", 2)["theta_events"] is None


def test_simulate_hands_the_threshold_to_the_accumulator_and_the_file(nsof_lib, monkeypatch, tmp_path):
    from nsof import accumulator as A  # noqa: N812
    seen = []

    class Stub:
        split = False

        def __init__(self, H, W, *a, **kw):  # noqa: N803
            seen.append(kw)
            self.shape = (H, W)

        def step(self, *a, **k):
            pass

        def snapshots(self):
            return [np.ones((1,) + self.shape, F)]

        def w(self, which=0):
            return np.zeros(self.shape, F)

        def close(self):
            pass
    monkeypatch.setattr(A, "Accumulator", Stub)
    ev = (np.int16([1, 3]), np.int16([1, 2]), np.int8([1, 0]), np.int64([0, 1500]))
    A.simulate(ev, version=1, sensor_size=(4, 4), out_prefix=tmp_path / "run.x", theta_events=3)
    assert seen[-1]["theta_events"] == 3
    with gzip.open(tmp_path / "run.V1.json.gz", "rt") as fp:
        assert json.load(fp)["theta_events"] == 3


def test_forwarding_functions_carry_the_keyword(nsof_lib):
    from nsof import accumulator, dist, pipeline
    fns = [pipeline.events_to_rois, pipeline.events_to_rois_host, pipeline.events_to_roi_flows,
           pipeline.events_to_flow_sequence, pipeline.events_to_flow_sequence_sharded, dist.accumulator_band]
    for fn in fns + [accumulator.simulate, accumulator.Accumulator.__init__]:
        prm = inspect.signature(fn).parameters
        assert "theta_events" in prm and prm["theta_events"].default is None, fn.__name__
    for fn in (accumulator.simulate, accumulator.Accumulator.__init__):
        assert inspect.signature(fn).parameters["theta_events"].kind is inspect.Parameter.KEYWORD_ONLY
    assert isinstance(accumulator.Accumulator.theta_events, property) and accumulator.Accumulator.theta_events.fset is None


def test_pipeline_forwards_the_threshold_unchanged(nsof_lib, monkeypatch):
    import torch

    from nsof import accumulator, dist, gating, pipeline
    seen = []

    class Stop(Exception):
        pass

    class Stub:
        def __init__(self, *a, **kw):
            seen.append(kw)
            raise Stop
    monkeypatch.setattr(pipeline, "Accumulator", Stub)
    monkeypatch.setattr(accumulator, "Accumulator", Stub)
    monkeypatch.setattr(torch, "empty", lambda *a, **k: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    rng = np.random.default_rng(0)
    n = 400
    x, y = rng.integers(0, 32, n).astype(np.int16), rng.integers(0, 32, n).astype(np.int16)
    p, t = rng.integers(0, 2, n).astype(np.int8), np.sort(rng.integers(0, 100_000, n)).astype(np.int64)
    cfg = gating.GatingConfig(MEMSIZE=8)

    class Ctx:
        device = 0
    calls = [lambda: pipeline.events_to_rois(x, y, p, t, (32, 32), cfg, ctx=Ctx(), theta_events=4),
             lambda: pipeline.events_to_rois_host(x, y, p, t, (32, 32), cfg, ctx=Ctx(), theta_events=4),
             lambda: pipeline.events_to_roi_flows(x, y, p, t, (32, 32), cfg, snapshot_every=10, ctx=Ctx(), theta_events=4),
             lambda: pipeline.events_to_flow_sequence(x, y, p, t, (32, 32), snapshot_every=10, ctx=Ctx(), theta_events=4)]
    monkeypatch.setattr(dist, "events_to_flow_sharded",
                        lambda x, y, p, t, hw, slice_us, every, band_frames, flow_of_frames, **k:
                        band_frames(x, y, p, t, np.arange(3), hw, every, 2))
    monkeypatch.setattr(torch.distributed, "is_initialized", lambda: False)
    calls.append(lambda: pipeline.events_to_flow_sequence_sharded(x, y, p, t, (32, 32), snapshot_every=10, ctx=Ctx(),
                                                                  theta_events=4))
    band = dist.accumulator_band(1, "split", -6.0, 0.0, ctx=Ctx(), theta_events=4)
    calls.append(lambda: band(x, y, p, t, np.arange(3), (32, 32), (np.zeros(2, np.int64), np.zeros(2, np.int64))))
    for i, call in enumerate(calls):
        with pytest.raises(Stop):
            call()
        assert len(seen) == i + 1 and seen[-1]["theta_events"] == 4, i
    with pytest.raises(Stop):
        pipeline.events_to_rois_host(x, y, p, t, (32, 32), cfg, ctx=Ctx())
    assert seen[-1]["theta_events"] is None
