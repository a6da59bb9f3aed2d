"""GPU: ``pipeline.events_variability_dev`` -- what a device spread does to the ROIs of an event stream: the nominal run on
the existing path, all trials in one trial run, gate statistics and one gating call over every (trial, snapshot) map.

The stream is the 240x320 one of tests/test_gating.py's config-3 tests (a moving box over background events, 160 slices of
1 ms, a snapshot every 40, 20 x 20 blocks, THRES 240).  ``silent_v`` = 0.5 V lies above von: idle pixels leak towards Roff, so
the gate is not trivially open (the every-pixel form of the trial run); ``silent_v`` = 0 is the dead-zone form."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H, W, EVERY, TRIALS = 240, 320, 40, 4
SIGMA = {k: 0.1 for k in ("kon", "koff", "Ron", "Roff")}


@pytest.fixture(scope="module")
def stream(nsof_lib):
    from nsof import synth
    return synth.make_events(7, W, H, n_background=3000, duration_us=160_000, box=(40, 30), speed_pps=500.0)


def config(nsof_lib, flag):
    from nsof import gating
    return gating.GatingConfig(MEMSIZE=20, EXTEND_HEIGHT_UPPER=10, EXTEND_HEIGHT_LOWER=10, EXTEND_WIDTH_LEFT=10, EXTEND_WIDTH_RIGHT=10,
                               THRES=240, FLAG=flag, farneback_params=nsof_lib.farneback.PARAMS_A)


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("rel_sigma", [{}, {k: 0.0 for k in SIGMA}], ids=["empty", "zeros"])
def test_no_spread_reproduces_the_nominal_run(nsof_lib, ctx, stream, rel_sigma):
    from nsof import pipeline
    out = host(pipeline.events_variability_dev(*stream, (H, W), config(nsof_lib, 1), rel_sigma, TRIALS, slice_us=1000, silent_v=0.5,
                                               snapshot_every=EVERY, ctx=ctx))
    assert out["nominal"].shape == (4, H // 20, W // 20) and out["stacks"].shape == (TRIALS,) + out["nominal"].shape
    for t in range(TRIALS):
        assert np.array_equal(out["stacks"][t].view(np.int64), out["nominal"].view(np.int64)), t
    assert not out["flips"].any() and set(np.unique(out["counts"])) <= {0, TRIALS}
    assert (out["counts"] == TRIALS).any() and (out["counts"] == 0).any()            # the gate is neither shut nor wide open
    assert np.array_equal(out["p_gate"], out["counts"] / TRIALS)
    # the same rectangles in every trial (a table's rows beyond its count are not written)
    assert out["rect_counts"].any() and all(np.array_equal(out["rect_counts"][t], out["rect_counts"][0]) for t in range(TRIALS))
    for k, c in enumerate(out["rect_counts"][0]):
        assert all(np.array_equal(out["rects"][t, k, :c], out["rects"][0, k, :c]) for t in range(TRIALS)), k


@pytest.mark.parametrize("silent_v", [0.5, 0.0])
@pytest.mark.parametrize("flag", [1, 2])
def test_ten_percent_spread(nsof_lib, ctx, stream, flag, silent_v):
    from nsof import gating, pipeline
    from nsof.accumulator import Accumulator, slice_index_array, variability_maps
    cfg = config(nsof_lib, flag)
    out = host(pipeline.events_variability_dev(*stream, (H, W), cfg, SIGMA, TRIALS, seed=5, slice_us=1000, silent_v=silent_v,
                                               snapshot_every=EVERY, ctx=ctx))
    stacks, nominal = out["stacks"], out["nominal"]
    n = nominal.shape[0]
    assert n == 4 and stacks.shape == (TRIALS, n, H // 20, W // 20)
    # the nominal stack is the existing pipeline's
    rois = pipeline.events_to_rois(*stream, (H, W), cfg, slice_us=1000, silent_v=silent_v, snapshot_every=EVERY, ctx=ctx)
    assert all(np.array_equal(rois[k][0], gating.current_to_gray(nominal[k])) for k in range(n))
    # the gate statistics are the host's on the downloaded stacks
    counts, flips = gating.gate_stats(stacks, nominal, cfg.THRES)
    assert np.array_equal(out["counts"], counts) and np.array_equal(out["flips"], flips)
    assert np.array_equal(out["p_gate"], counts / TRIALS)
    # the rectangles are the host gating of each downloaded map (events_to_rois_host's: gray, threshold, components, boxes)
    for t in range(TRIALS):
        for k in range(n):
            g = gating.current_to_gray(stacks[t, k])
            tp = gating.update_transition_pic(g, np.zeros((H // 20, W // 20)), cfg.THRES).astype(np.uint8)
            nl, _, stats, _ = gating.connectedComponentsWithStats(tp, cfg.CONNECT)
            rb = [gating._roi(*[int(v) for v in stats[i, :4]], W, H, cfg.MEMSIZE, cfg.MEMSIZE, cfg) for i in range(1, nl)]
            if flag == 2 and rb:
                rb = [(min(r[0] for r in rb), min(r[1] for r in rb), max(r[2] for r in rb), max(r[3] for r in rb))]
            c = int(out["rect_counts"][t, k])
            assert [tuple(int(v) for v in r) for r in out["rects"][t, k, :c]] == rb, (t, k)
    # every trial's stack is the block currents of a single-array run with that trial's maps
    maps = variability_maps(H, W, SIGMA, None, 5, trials=TRIALS)
    for t in range(TRIALS):
        acc = Accumulator(H, W, 1, "split", -6.0, silent_v, ctx=ctx, param_maps={k: v[t] for k, v in maps.items()})
        try:
            acc.step(*stream, slice_index_array(stream[3], 1000), snap_every=EVERY)
            assert acc.snapshot_count() == n
            for k in range(n):
                assert np.array_equal(acc.block_current(cfg.MEMSIZE, snapshot=k).view(np.int64), stacks[t, k].view(np.int64)), (t, k)
        finally:
            acc.close()
    assert not np.array_equal(stacks[0], stacks[1])
    if silent_v == 0.5:
        assert flips.any() and out["rect_counts"].any()        # a 10 % spread moves the gate of this stream
