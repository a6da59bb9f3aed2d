"""GPU: scheme 1's event-count threshold (THETA_EVENTS) on every accumulator route.

The yardstick is structural and exact: a run at threshold theta on (events, bounds) must equal, ``np.array_equal``, the
threshold-1 run on the FILTERED stream -- the same events without every (pixel, slice) cell that holds fewer than theta
events, the same slices re-indexed (``accum_theta_ref.filter_stream``, checked against the NumPy restatement in
tests/test_accum_theta_cpu.py).  Both runs use the library's own arithmetic, so no tolerance enters.  Each test first
asserts that its stream has cells with theta - 1, theta and more than theta events: the two event sets differ, and a
library that ignores theta fails.  Only the comparison with the reference's own fixture (tests/golden/accum_theta_v1.npz)
carries tolerances: those of tests/test_accum_gpu.py."""
import ctypes as C
import gzip
import json

import numpy as np
import pytest

import accum_theta_ref as T
from conftest import golden_path

pytestmark = pytest.mark.gpu

W_ATOL = 5e-7       # tests/test_accum_gpu.py
R_RTOL = 2e-6
F = np.float32
THETAS = (2, 3, 5, 200)
INT32_MAX = 2**31 - 1
_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def make_stream(seed, W, H, n_slices, thetas=THETAS):  # noqa: N803
    """A time-sorted stream of ``n_slices`` 1000-us slices with explicit bounds: random background with a third of it on a
    small patch (cells of 2 .. 6 events), some empty slices, and -- in the sensor's last column, which the background
    avoids -- one cell each of theta - 1, theta and theta + 3 events for every theta.  The first and the last slice hold a
    cell of 8 events at t = 0 and at the stream's end, so a filtered copy keeps the time span."""
    rng = np.random.default_rng(seed)
    n_background = 60 * n_slices
    sl = rng.integers(0, n_slices, n_background)
    x = rng.integers(0, W - 1, n_background)
    y = rng.integers(0, H, n_background)
    k = n_background // 3
    x[:k] = rng.integers(10, 14, k)
    y[:k] = rng.integers(20, 23, k)
    empty = (13, 14, n_slices // 2)
    live = ~np.isin(sl, empty)
    sl, x, y = sl[live], x[live], y[live]
    xs, ys, ss = [x], [y], [sl]
    row = 0
    for th in thetas:
        for n in (th - 1, th, th + 3):
            s = int(rng.choice([v for v in range(1, n_slices - 1) if v not in empty]))
            xs.append(np.full(n, W - 1)); ys.append(np.full(n, row)); ss.append(np.full(n, s))
            row += 1
    assert row <= H - 2
    for s, yy in ((0, H - 2), (n_slices - 1, H - 1)):
        xs.append(np.full(8, W - 1)); ys.append(np.full(8, yy)); ss.append(np.full(8, s))
    x, y, sl = np.concatenate(xs), np.concatenate(ys), np.concatenate(ss)
    t = sl * 1000 + rng.integers(1, 999, sl.size)
    t[-16:-8] = 0                                   # the first slice's planted cell opens the stream ...
    t[-8:] = n_slices * 1000 - 1                    # ... and the last one's closes it
    order = np.argsort(t, kind="stable")
    x, y, t = x[order].astype(np.int16), y[order].astype(np.int16), t[order].astype(np.int64)
    p = rng.integers(0, 2, x.size).astype(np.int8)
    bounds = np.searchsorted(t, np.arange(0, (n_slices + 1) * 1000, 1000)).astype(np.int64)
    assert bounds[-1] == x.size
    return (x, y, p, t), bounds


def probe(ev, bounds, theta, W):  # noqa: N803
    """The stream has cells just below, at and above the threshold; returns the filtered twin."""
    _, c = T.cell_counts(ev[0], ev[1], bounds, W)
    assert (c == theta - 1).any() and (c == theta).any() and (c > theta).any(), theta
    evf, bf = T.filter_stream(*ev, bounds, theta, W)
    assert 0 < evf[0].size < ev[0].size
    return evf, bf


def stream_and_twins(W, H, n_slices=100):  # noqa: N803
    def make():
        ev, bounds = make_stream(100 + W, W, H, n_slices)
        return ev, bounds, {th: probe(ev, bounds, th, W) for th in THETAS}
    return cached(("stream", W, H, n_slices), make)


def run(nsof_lib, ctx, ev, bounds, hw, theta=None, dense=None, active_v=-6.0, silent_v=0.0, snap_every=0):
    kw = {} if theta is None else dict(theta_events=theta)
    acc = nsof_lib.Accumulator(hw[0], hw[1], 1, "split", active_v, silent_v, ctx=ctx, dense=dense, **kw)
    try:
        assert acc.theta_events == (1 if theta is None else theta)
        acc.step(*ev, bounds, snap_every=snap_every)
        return acc.w(0), acc.snapshots()[0]
    finally:
        acc.close()


# ---- update forms ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", THETAS)
@pytest.mark.parametrize("dense", [False, True, None], ids=["event_pixel", "every_pixel", "auto"])
def test_update_forms_equal_the_filtered_twin(nsof_lib, ctx, dense, theta):
    for W, H in ((64, 48), (37, 29)):  # noqa: N806
        ev, bounds, twins = stream_and_twins(W, H)
        evf, bf = twins[theta]
        for silent_v in (0.0, 0.5):
            for snap_every in (0, 7):
                kw = dict(dense=dense, silent_v=silent_v, snap_every=snap_every)
                w, snaps = run(nsof_lib, ctx, ev, bounds, (H, W), theta, **kw)
                w1, snaps1 = cached(("twin", W, H, theta, dense, silent_v, snap_every),
                                    lambda: run(nsof_lib, ctx, evf, bf, (H, W), None, **kw))
                tag = (W, H, silent_v, snap_every)
                assert np.array_equal(w, w1), tag
                assert snaps.shape == snaps1.shape and snaps.shape[0] == (0 if not snap_every else (99 // 7) + 1), tag
                assert np.array_equal(snaps, snaps1), tag
                # and the threshold did something: the plain run on the unfiltered stream differs
                w0, _ = cached(("plain", W, H, silent_v), lambda: run(nsof_lib, ctx, ev, bounds, (H, W), None, silent_v=silent_v))
                assert not np.array_equal(w, w0), tag


def test_update_forms_agree_with_each_other(nsof_lib, ctx):
    ev, bounds, _ = stream_and_twins(37, 29)
    for theta in THETAS:
        a = run(nsof_lib, ctx, ev, bounds, (29, 37), theta, dense=False, snap_every=7)
        b = run(nsof_lib, ctx, ev, bounds, (29, 37), theta, dense=True, snap_every=7)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), theta


# ---- theta above every count -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [10**6, INT32_MAX])
@pytest.mark.parametrize("dense", [False, True, None], ids=["event_pixel", "every_pixel", "auto"])
def test_threshold_above_every_count_drives_nothing(nsof_lib, ctx, dense, theta):
    ev, bounds, _ = stream_and_twins(64, 48)
    _, c = T.cell_counts(ev[0], ev[1], bounds, 64)
    assert c.max() < theta
    w, snaps = run(nsof_lib, ctx, ev, bounds, (48, 64), theta, dense=dense, snap_every=7)
    assert np.array_equal(w.view(np.int32), np.full((48, 64), 0.5, F).view(np.int32))   # wini everywhere, bit for bit
    assert (snaps == snaps[0, 0, 0]).all()
    # with the leak: the run without events
    none = tuple(a[:0] for a in ev)
    w, snaps = run(nsof_lib, ctx, ev, bounds, (48, 64), theta, dense=dense, silent_v=0.5, snap_every=7)
    w0, snaps0 = run(nsof_lib, ctx, none, np.zeros_like(bounds), (48, 64), None, dense=dense, silent_v=0.5, snap_every=7)
    assert np.array_equal(w, w0) and np.array_equal(snaps, snaps0)
    assert (w < 0.5).all()


# ---- the reference's fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,theta", [("dead", 2), ("dead", 3), ("dead", 5), ("leak", 2), ("leak", 3)])
def test_simulate_vs_reference_fixture(nsof_lib, ctx, tmp_path, name, theta):
    d = np.load(golden_path("accum_theta_v1.npz"))
    ev = tuple(d[f"{name}_{k}"] for k in "xypt")
    out = nsof_lib.simulate(ev, version=1, slice_us=int(d["slice_us"]), active_v=float(d[f"{name}_active_v"]),
                            silent_v=float(d[f"{name}_silent_v"]), sensor_size=(48, 64), ctx=ctx, theta_events=theta,
                            out_prefix=tmp_path / "run.x" if theta == 5 else None)
    w_ref, r_ref = d[f"{name}_th{theta}_w_final"], d[f"{name}_th{theta}_resistances"]
    assert out["resistances"].shape[0] == int(d[f"{name}_n_snapshots"])
    dw = float(np.abs(out["w_final"] - w_ref).max())
    dr = float((np.abs(out["resistances"][d["snap_idx"]] - r_ref) / r_ref).max())
    print(f"{name} theta {theta}: max |dw| {dw:.3g}, max rel dR {dr:.3g}")
    assert dw <= W_ATOL
    assert dr <= R_RTOL
    if theta == 5:
        with gzip.open(tmp_path / "run.V1.json.gz", "rt") as fp:
            meta = json.load(fp)
        assert meta["theta_events"] == 5 and meta["scheme"] == "boxcar" and meta["refractory_us"] is None


# ---- a hand-built stream of 200 slices ---------------------------------------------------------------------------------
PIX_NEVER, PIX_FLOOD, PIX_TWICE = (3, 2), (40, 7), (21, 30)   # (x, y)


def hand_stream(theta, W=64, H=48, n_slices=200):  # noqa: N803
    """(x, y) -> {slice: events}: a pixel that collects theta - 1 events in slices 5, 37, 69 and 21 (never enough in one
    slice: counters left over from an earlier group would fire it); a pixel with 5000 events in slice 70 and theta in slice
    75 (saturation; one list entry); a pixel that reaches theta in slices 100 and 101 of one group; a few background cells
    around the threshold; every other slice empty."""
    cells = {PIX_NEVER: {5: theta - 1, 37: theta - 1, 69: theta - 1, 21: theta - 1},
             PIX_FLOOD: {70: 5000, 75: theta},
             PIX_TWICE: {100: theta, 101: theta + 1},
             (50, 40): {0: theta + 2, 120: theta - 1, 121: theta, 199: theta + 2},
             (63, 47): {150: theta, 151: theta - 1, 183: 1},
             (0, 0): {160: 1, 161: theta, 162: 2 * theta}}
    rng = np.random.default_rng(theta)
    xs, ys, ss = [], [], []
    for (px, py), per in cells.items():
        for s, n in per.items():
            xs.append(np.full(n, px)); ys.append(np.full(n, py)); ss.append(np.full(n, s))
    x, y, sl = np.concatenate(xs), np.concatenate(ys), np.concatenate(ss)
    t = sl * 1000 + rng.integers(0, 1000, sl.size)
    order = np.argsort(t, kind="stable")
    x, y, t = x[order].astype(np.int16), y[order].astype(np.int16), t[order].astype(np.int64)
    p = rng.integers(0, 2, x.size).astype(np.int8)
    bounds = np.searchsorted(t, np.arange(0, (n_slices + 1) * 1000, 1000)).astype(np.int64)
    return (x, y, p, t), bounds


def step_n(w, n, active_v=-6.0):
    import accum_params_ref as R  # noqa: N812
    w = np.array([w], F)
    for _ in range(n):
        w = R.update_state(w, np.array([active_v], F))
    return w[0]


@pytest.mark.parametrize("theta", [2, 3, 7])
def test_hand_built_stream(nsof_lib, ctx, theta):
    ev, bounds = hand_stream(theta)
    evf, bf = probe(ev, bounds, theta, 64)
    assert np.diff(bounds).tolist().count(0) > 150          # most slices are empty
    want = None
    for dense in (False, True, None):
        w, _ = run(nsof_lib, ctx, ev, bounds, (48, 64), theta, dense=dense)
        w1, _ = run(nsof_lib, ctx, evf, bf, (48, 64), None, dense=dense)
        assert np.array_equal(w, w1), dense
        assert w[PIX_NEVER[1], PIX_NEVER[0]] == F(0.5), dense
        assert w[PIX_FLOOD[1], PIX_FLOOD[0]] != F(0.5) and w[PIX_TWICE[1], PIX_TWICE[0]] != F(0.5)
        # driven cells per pixel: two for the flooded pixel (5000 events are one pulse) and for the pixel that reaches theta twice
        moved = w != F(0.5)
        assert int(moved.sum()) == 5, dense
        assert w[PIX_FLOOD[1], PIX_FLOOD[0]] == w[PIX_TWICE[1], PIX_TWICE[0]]
        assert abs(float(w[PIX_FLOOD[1], PIX_FLOOD[0]]) - float(step_n(0.5, 2))) <= 2.4e-7   # two steps of the project's one-step bound
        want = w if want is None else want
        assert np.array_equal(w, want)


# ---- sub-ranges, repeats, reset, a changed threshold -------------------------------------------------------------------
def set_threshold(acc, theta):
    return acc.ctx._lib.nsof_accum_set_event_threshold(acc._p, int(theta))


@pytest.mark.parametrize("dense", [False, True, None], ids=["event_pixel", "every_pixel", "auto"])
def test_subranges_repeats_reset_and_threshold_changes(nsof_lib, ctx, dense):
    ev, bounds, twins = stream_and_twins(64, 48, 200)
    acc = nsof_lib.Accumulator(48, 64, 1, "split", -6.0, 0.0, ctx=ctx, dense=dense, theta_events=3)
    twin = {th: nsof_lib.Accumulator(48, 64, 1, "split", -6.0, 0.0, ctx=ctx, dense=dense) for th in (2, 3)}
    plain = nsof_lib.Accumulator(48, 64, 1, "split", -6.0, 0.0, ctx=ctx, dense=dense)   # never sees the setter
    try:
        acc.set_events(*ev, bounds)
        plain.set_events(*ev, bounds)
        for th in (2, 3):
            twin[th].set_events(*twins[th][0], twins[th][1])
        states = []
        for first, n in ((40, 50), (40, 50), (0, 200)):
            acc.run(first, n)
            twin[3].run(first, n)
            states.append(acc.w(0))
            assert np.array_equal(states[-1], twin[3].w(0)), (first, n)
        assert not np.array_equal(states[0], states[1]) and not np.array_equal(states[1], states[2])
        acc.reset()
        twin[3].reset()
        assert np.array_equal(acc.w(0), np.full((48, 64), 0.5, F))
        acc.run(0, 200, 7)
        twin[3].run(0, 200, 7)
        w3 = acc.w(0)
        assert np.array_equal(w3, twin[3].w(0)) and np.array_equal(acc.snapshots()[0], twin[3].snapshots()[0])
        assert np.array_equal(w3, run(nsof_lib, ctx, ev, bounds, (48, 64), 3, dense=dense)[0])   # a fresh accumulator
        # 3 -> 1: the kernels the library always ran, on state left by the counting ones
        assert set_threshold(acc, 1) == 0 and acc.theta_events == 1
        acc.reset()
        acc.run(0, 200)
        plain.run(0, 200)
        assert np.array_equal(acc.w(0), plain.w(0)) and not np.array_equal(acc.w(0), w3)
        # 1 -> 2, continuing from that state: other field widths, other group sizes
        assert set_threshold(acc, 2) == 0 and acc.theta_events == 2
        twin[2].load_state(dict(w=acc.w(0), slice_counter=200))
        acc.run(17, 120)
        twin[2].run(17, 120)
        assert np.array_equal(acc.w(0), twin[2].w(0)) and not np.array_equal(acc.w(0), plain.w(0))
    finally:
        for a in (acc, plain, *twin.values()):
            a.close()


# ---- frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames_path", [None, "copy_patch"])
@pytest.mark.parametrize("every", [1, 33, 64])
@pytest.mark.parametrize("mode,active_v", [("state", -6.0), ("current", -3.0)])
def test_frames_equal_the_filtered_twin_and_per_interval_surfaces(nsof_lib, ctx, torch_dev, mode, active_v, every, frames_path):
    """64x48: at threshold 1 the tile walk applies (the twin takes it by default), with a threshold copy + patch or the
    per-interval passes do -- the same bytes.  ("current" is 255 for every w >= 0.29 and so for the initial 0.5: that mode
    starts from a ramp of states below, where every pulse shows in the frame.)"""
    import torch
    ev, bounds, twins = stream_and_twins(64, 48, 200)
    n_frames = min(200 // every, 40)
    w0 = None if mode == "state" else np.linspace(0.0, 0.28, 48 * 64, dtype=F).reshape(48, 64)

    def start(a):
        if w0 is None:
            a.reset()
        else:
            a.load_state(dict(w=w0, slice_counter=0))
    for theta in (2, 5):
        evf, bf = twins[theta]
        for dense in (None, False, True):
            kw = dict(ctx=ctx, dense=dense, frames_path=frames_path)
            acc = nsof_lib.Accumulator(48, 64, 1, "split", active_v, 0.0, theta_events=theta, **kw)
            twin = nsof_lib.Accumulator(48, 64, 1, "split", active_v, 0.0, **kw)
            try:
                acc.set_events(*ev, bounds)
                twin.set_events(*evf, bf)
                start(acc)
                start(twin)
                fr = [torch.full((n_frames, 48, 64), 7, dtype=torch.uint8, device=torch_dev) for _ in range(3)]
                acc.run_frames(0, n_frames, every, fr[0], mode=mode)
                twin.run_frames(0, n_frames, every, fr[1], mode=mode)
                ctx.synchronize()
                w = acc.w(0)
                assert np.array_equal(w, twin.w(0)), (theta, dense)
                start(acc)
                for k in range(n_frames):
                    acc.run_surface(k * every, every, fr[2][k], mode=mode)
                ctx.synchronize()
                a, b, c = (f.cpu().numpy() for f in fr)
                assert np.array_equal(a, b), (theta, dense)
                assert np.array_equal(a, c) and np.array_equal(w, acc.w(0)), (theta, dense)
                assert len(np.unique(a)) >= 2 and not np.array_equal(a[0], a[-1])   # frames that say something
            finally:
                acc.close()
                twin.close()


# ---- setter and getter -------------------------------------------------------------------------------------------------
def test_setter_and_getter(nsof_lib, ctx):
    lib = ctx._lib
    ev, bounds, twins = stream_and_twins(64, 48)
    acc = nsof_lib.Accumulator(48, 64, 1, "split", -6.0, 0.0, ctx=ctx)
    try:
        th = C.c_int(-1)
        assert lib.nsof_accum_get_event_threshold(acc._p, C.byref(th)) == 0 and th.value == 1 == acc.theta_events
        for good in (3, INT32_MAX, 1, 5):
            assert lib.nsof_accum_set_event_threshold(acc._p, good) == 0
            assert lib.nsof_accum_get_event_threshold(acc._p, C.byref(th)) == 0 and th.value == good == acc.theta_events
        for bad in (0, -3):
            assert lib.nsof_accum_set_event_threshold(acc._p, bad) == nsof_lib._lib.NSOF_EINVAL
            with pytest.raises(nsof_lib.error) as e:
                ctx.check(nsof_lib._lib.NSOF_EINVAL, "set_event_threshold")
            assert str(bad) in str(e.value)
            assert acc.theta_events == 5
        assert lib.nsof_accum_get_event_threshold(acc._p, None) == nsof_lib._lib.NSOF_EINVAL
        acc.step(*ev, bounds)                              # still usable, still at 5
        assert np.array_equal(acc.w(0), run(nsof_lib, ctx, *twins[5], (48, 64), None)[0])
    finally:
        acc.close()
    two = nsof_lib.Accumulator(48, 64, 2, "split", -6.0, 0.0, ctx=ctx)
    try:
        assert lib.nsof_accum_set_event_threshold(two._p, 1) == 0 and two.theta_events == 1
        assert lib.nsof_accum_set_event_threshold(two._p, 2) == nsof_lib._lib.NSOF_EINVAL and two.theta_events == 1
        with pytest.raises(nsof_lib.error) as e:
            ctx.check(nsof_lib._lib.NSOF_EINVAL, "set_event_threshold")
        assert "2" in str(e.value) and "scheme 2" in str(e.value)
    finally:
        two.close()
    with pytest.raises(nsof_lib.error):
        nsof_lib.Accumulator(48, 64, 2, "split", -6.0, 0.0, ctx=ctx, theta_events=2)


# ---- forwarding --------------------------------------------------------------------------------------------------------
def test_pipeline_and_band_forward_the_threshold(nsof_lib, ctx):
    from nsof import dist, gating, pipeline
    from nsof.accumulator import slice_index_array
    ev, bounds, twins = stream_and_twins(64, 48)
    evf, bf = twins[2]
    # the time-sliced routes cut the stream themselves: the filtered copy must keep the grid
    assert np.array_equal(slice_index_array(ev[3], 1000), bounds) and np.array_equal(slice_index_array(evf[3], 1000), bf)
    cfg = gating.GatingConfig(MEMSIZE=8, EXTEND_HEIGHT_UPPER=4, EXTEND_HEIGHT_LOWER=4, EXTEND_WIDTH_LEFT=4,
                              EXTEND_WIDTH_RIGHT=4, THRES=240, FLAG=1)
    for fn in (pipeline.events_to_rois, pipeline.events_to_rois_host):
        kw = dict(slice_us=1000, silent_v=0.5, snapshot_every=30, ctx=ctx)
        a = fn(*ev, (48, 64), cfg, theta_events=2, **kw)
        b = fn(*evf, (48, 64), cfg, **kw)
        plain = fn(*ev, (48, 64), cfg, **kw)
        assert len(a) == len(b) == 4
        for (ga, ra), (gb, rb) in zip(a, b):
            assert np.array_equal(ga, gb) and [tuple(r) for r in ra] == [tuple(r) for r in rb]
        assert any(not np.array_equal(ga, gp) for (ga, _), (gp, _) in zip(a, plain))
    times = (np.zeros(100, np.int64), np.zeros(100, np.int64))   # scheme 1 reads no slice times
    wa = dist.accumulator_band(1, "split", -6.0, 0.0, ctx=ctx, theta_events=2)(*ev, bounds, (48, 64), times)
    wb = dist.accumulator_band(1, "split", -6.0, 0.0, ctx=ctx)(*evf, bf, (48, 64), times)
    wp = dist.accumulator_band(1, "split", -6.0, 0.0, ctx=ctx)(*ev, bounds, (48, 64), times)
    assert np.array_equal(wa, wb) and not np.array_equal(wa, wp)
