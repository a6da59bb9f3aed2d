"""GPU: accumulator trajectories bit for bit against the oracle's correctly rounded mode, and the edges of
nsof_accum_run_frames' two event-driven paths (the tile walk and copy + patch).

The update is a pure float32 function of w for a fixed V and each pixel's trajectory is serial, so a device that rounds
its powers correctly outside the device band (tests/test_accum_cr_gpu.py) reproduces the correctly rounded oracle
exactly on any run in which the oracle reports no step inside that band.  Each test first asserts that (fixed seeds),
then demands np.array_equal.  The tolerance checks of test_accum_gpu.py stay as they are."""
import numpy as np
import pytest

from conftest import golden_path

pytestmark = pytest.mark.gpu

F = np.float32
CASES = ["v1", "v2_split", "v2_magnitude", "v1_leak", "v2_split_bias", "v1_exact", "v2_split_pm1"]


def _same(a, b):
    return a.shape == b.shape and np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


@pytest.mark.parametrize("name", CASES)
def test_golden_streams_exact(nsof_lib, ctx, oracle, name):
    """Every golden stream: w_final and every snapshot's resistances.  Two of the streams (v1_leak: 1 step,
    v2_split_bias: 5 steps) do pass through the device band; the pixels whose trajectory did are left out there (the
    oracle marks them), every other pixel is held bit for bit."""
    d = np.load(golden_path(f"accum_sim_{name}.npz"))
    H, W = d["w_final"].shape
    ref = oracle.accum_simulate(d["x"], d["y"], d["p"], d["t"], H, W, int(d["version"]), str(d["polarity"]),
                                int(d["slice_us"]), float(d["active_v"]), float(d["silent_v"]), rounding="correct")
    assert ref["band"] == {"v1_leak": 1, "v2_split_bias": 5}.get(name, 0)
    out = nsof_lib.simulate((d["x"], d["y"], d["p"], d["t"]), version=int(d["version"]), slice_us=int(d["slice_us"]),
                            active_v=float(d["active_v"]), silent_v=float(d["silent_v"]), polarity=str(d["polarity"]),
                            sensor_size=(H, W), ctx=ctx)
    for k, m in (("w_final", "band_px"), ("resistances", "band_px"), ("w_final_b", "band_px_b"),
                 ("resistances_b", "band_px_b")):
        assert (k in out) == (k in ref), k
        if k in ref:
            keep = ~ref[m]
            assert keep.sum() >= H * W - ref["band"]
            assert out[k].shape == ref[k].shape and _same(out[k][..., keep], ref[k][..., keep]), (name, k)


def test_dense_groups_of_64_slices_exact(nsof_lib, ctx, oracle):
    """The groups of up to 64 slices of test_dense_groups_of_64_slices, both updates, and the leaking every-pixel run."""
    from nsof import synth
    from nsof.accumulator import Accumulator, slice_index_array
    H, W = 90, 131
    x, y, p, t = synth.make_events(17, W, H, 9000, 150_000, box=(20, 16))
    idx = slice_index_array(t, 1000)
    n = len(idx) - 1
    for silent in (0.0, 0.5):
        ref = oracle.accum_simulate(x, y, p, t, H, W, 1, "split", 1000, -6.0, silent, rounding="correct")
        assert ref["band"] == 0
        for dense in ((False, True) if silent == 0.0 else (None,)):
            acc = Accumulator(H, W, 1, "split", -6.0, silent, ctx=ctx, dense=dense)
            try:
                acc.set_events(x, y, p, t, idx)
                acc.run(0, 70)
                acc.run(70, 33)
                acc.run(103, n - 103)
                assert _same(acc.w(), ref["w_final"]), (silent, dense)
            finally:
                acc.close()


def test_full_size_leak_run_exact(nsof_lib, ctx, oracle):
    """3840 x 2160, silent voltage 0.4 (every pixel leaks in every slice): 8 slices == the correctly rounded oracle."""
    from nsof import synth
    from nsof.accumulator import Accumulator, slice_index_array
    H, W = 2160, 3840
    x, y, p, t = synth.make_events(5, W, H, 40_000, 40_000, box=(400, 300))
    idx = slice_index_array(t, 1000)
    k = 8
    acc = Accumulator(H, W, 1, "split", -6.0, 0.4, ctx=ctx)
    try:
        acc.step(x, y, p, t, idx[:k + 1], snap_every=0)
        got = acc.w(0)
    finally:
        acc.close()
    w = np.full((H, W), 0.5, F)
    band = 0
    for s in range(k):
        V = np.full((H, W), 0.4, F)
        V[y[idx[s]:idx[s + 1]], x[idx[s]:idx[s + 1]]] = -6.0
        w, b = oracle.accum_update_state(w, V, rounding="correct")
        band += int(b.sum())
    assert band == 0
    assert _same(got, w)


def _refractory_edges(H, W, seed):
    """A scheme-2 stream whose pixels fire exactly 799, 800 and 801 us apart (both polarities), over a background."""
    from nsof import synth
    x, y, p, t = synth.make_events(seed, W, H, 3000, 60_000, box=(12, 9))
    xs, ys, ps, ts = [x], [y], [p], [t]
    for j, gap in enumerate((799, 800, 801)):
        for pol in (0, 1):
            tt = np.arange(137, 58_000, gap, dtype=np.int64)
            xs.append(np.full(tt.size, 3 + 4 * j + 2 * pol, np.int16))
            ys.append(np.full(tt.size, 2 + j, np.int16))
            ps.append(np.full(tt.size, pol, np.int8))
            ts.append(tt)
    x, y, p, t = (np.concatenate(a) for a in (xs, ys, ps, ts))
    o = np.argsort(t, kind="stable")
    return x[o].astype(np.int16), y[o].astype(np.int16), p[o].astype(np.int8), t[o]


def _tail_stream(H, W):
    from nsof import synth
    return synth.make_events(3, W, H, 4000, 70_000, box=(12, 9))


# case -> (H, W, stream, silent_v, dense).  The 37 x 45 sensor has 1665 pixels, 1665 % 4 == 1: the every-pixel update
# (k_update_all) ends in its scalar tail there, which no sensor with a pixel count divisible by 4 reaches.
_S2_CASES = {
    "edges": (40, 48, lambda: _refractory_edges(40, 48, 3), 0.0, None),
    "tail-list": (37, 45, lambda: _tail_stream(37, 45), 0.0, False),       # event-pixel update (k_update_list)
    "tail-all-skip": (37, 45, lambda: _tail_stream(37, 45), 0.0, True),    # every-pixel, untouched quads skipped
    "tail-all-leak": (37, 45, lambda: _tail_stream(37, 45), 0.3, None),    # every-pixel, all slices replayed
}
_S2_REFS = {}


@pytest.mark.parametrize("polarity,case", [pytest.param(pol, case, id=pol if case == "edges" else f"{pol}-{case}")
                                           for case in _S2_CASES for pol in ("split", "magnitude")])
def test_scheme2_refractory_edges_exact(nsof_lib, ctx, oracle, polarity, case):
    H, W, stream, silent_v, dense = _S2_CASES[case]
    x, y, p, t = stream()
    key = (H, W, polarity, silent_v)   # the list and the every-pixel update of one run share its reference
    if key not in _S2_REFS:
        _S2_REFS[key] = oracle.accum_simulate(x, y, p, t, H, W, 2, polarity, 1000, -6.0, silent_v, rounding="correct")
    ref = _S2_REFS[key]
    assert ref["band"] == 0
    out = nsof_lib.simulate((x, y, p, t), version=2, slice_us=1000, active_v=-6.0, silent_v=silent_v, polarity=polarity,
                            sensor_size=(H, W), ctx=ctx, dense=dense)
    for k in ("w_final", "resistances", "w_final_b", "resistances_b"):
        assert (k in out) == (k in ref), k
        if k in ref:
            assert _same(out[k], ref[k]), k


@pytest.mark.parametrize("version,polarity", [(1, "split"), (2, "split"), (2, "magnitude")])
def test_staged_and_resumed_runs_exact(nsof_lib, ctx, oracle, version, polarity):
    """set_events + run over two sub-ranges, checkpointed and resumed in a new accumulator == the oracle's one run."""
    from nsof import synth
    W, H = 96, 64
    x, y, p, t = synth.make_events(5, W, H, 20000, 300_000, box=(20, 12))
    idx = nsof_lib.accumulator.slice_index_array(t, 1000)
    n = len(idx) - 1
    ref = oracle.accum_simulate(x, y, p, t, H, W, version, polarity, 1000, -6.0, 0.0, rounding="correct")
    assert ref["band"] == 0
    a = nsof_lib.Accumulator(H, W, version, polarity, -6.0, 0.0, ctx=ctx)
    a.set_events(x, y, p, t, idx)
    cut = n // 3 + 5
    a.run(0, cut)
    states = [a.state(k) for k in range(2 if a.split else 1)]
    a.close()
    b = nsof_lib.Accumulator(H, W, version, polarity, -6.0, 0.0, ctx=ctx)
    try:
        for k, st in enumerate(states):
            b.load_state(st, k)
        b.set_events(x, y, p, t, idx)
        b.run(cut, n - cut)
        assert _same(b.w(0), ref["w_final"])
        if b.split:
            assert _same(b.w(1), ref["w_final_b"])
    finally:
        b.close()


def _ref_frames(oracle, x, y, idx, H, W, first, n_frames, every, active_v, silent_v, mode, w=None):
    """The correctly rounded oracle slice by slice: the surface after each interval, the final state, the band count."""
    w = np.full((H, W), 0.5, F) if w is None else w.copy()
    frames = np.empty((n_frames, H, W), np.uint8)
    band = 0
    for k in range(n_frames):
        for s in range(first + k * every, first + (k + 1) * every):
            V = np.full((H, W), silent_v, F)
            V[y[idx[s]:idx[s + 1]], x[idx[s]:idx[s + 1]]] = active_v
            w, b = oracle.accum_update_state(w, V, rounding="correct")
            band += int(b.sum())
        g, b = oracle.accum_surface_u8(w, mode)
        frames[k] = g
        band += int(b.sum())
    return frames, w, band


@pytest.mark.parametrize("mode", ["state", "current"])
def test_run_surface_exact(nsof_lib, ctx, oracle, torch_dev, mode):
    """run_surface (the dense update writes the frame) and run + surface_u8, both == the oracle's frames and state."""
    import torch
    from nsof import synth
    from nsof.accumulator import Accumulator, slice_index_array
    for (H, W, silent, dense) in [(77, 131, 0.0, True), (90, 202, 0.5, True), (120, 160, 0.0, False)]:
        x, y, p, t = synth.make_events(9, W, H, 6000, 80_000, box=(20, 16))
        idx = slice_index_array(t, 1000)
        want, w_ref, band = _ref_frames(oracle, x, y, idx, H, W, 0, 2, 33, -6.0, silent, mode)
        assert band == 0
        acc = Accumulator(H, W, 1, "split", -6.0, silent, ctx=ctx, dense=dense)
        try:
            acc.set_events(x, y, p, t, idx)
            buf = torch.zeros((2, H, W), dtype=torch.uint8, device=torch_dev)
            torch.cuda.synchronize()
            for k in range(2):
                acc.run_surface(k * 33, 33, buf[k], mode=mode)
            ctx.synchronize()
            assert np.array_equal(buf.cpu().numpy(), want), (H, W, silent, dense)
            assert _same(acc.w(), w_ref)
        finally:
            acc.close()


def test_row_bands_world_size_one_exact(nsof_lib, ctx, oracle):
    """nsof.dist.simulate_banded with the GPU accumulator on an RCCL group of one rank == the correctly rounded oracle."""
    import os

    import torch.distributed as dist
    from nsof import dist as nd
    from nsof import synth
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ["MASTER_PORT"] = str(29870 + os.getpid() % 40)
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    os.environ.setdefault("LOCAL_RANK", "0")
    W, H = 64, 47
    x, y, p, t = synth.make_events(11, W, H, 3000, 40_000, box=(12, 9))
    ref = oracle.accum_simulate(x, y, p, t, H, W, 1, "split", 1000, -6.0, 0.0, rounding="correct")
    assert ref["band"] == 0

    def band(xb, yb, pb, tb, idx_b, hw, slice_times):
        if hw[0] == 0:
            return np.zeros(hw, F)
        acc = nsof_lib.Accumulator(hw[0], hw[1], 1, "split", -6.0, 0.0, ctx=ctx)
        try:
            acc.step(xb, yb, pb, tb, idx_b)
            return acc.w()
        finally:
            acc.close()

    created = not dist.is_initialized()
    if created:
        dist.init_process_group("nccl")
    try:
        out = nd.simulate_banded(x, y, p, t, (H, W), 1000, band)
    finally:
        if created:
            dist.destroy_process_group()
    assert _same(out.numpy(), ref["w_final"])


# ---- run_frames edges ---------------------------------------------------------------------------------------------------
# nsof_accum_run_frames takes an event-driven path for scheme 1 with the silent voltage in the dead zone, dense not forced
# and every <= 64.  Of those, the TILE WALK (k_tile_bucket + k_tile_frames) needs tile_ok:
#     W % 16 == 0, row stride % 16 == 0, frame stride % 16 == 0, frames base 16-byte aligned, n_frames >= 2,
#     fewer than 2^31 events, at most 15000 tiles of 1024 pixels, and the path not set to "copy_patch";
# otherwise COPY + PATCH (k_frames_scatter_copy + k_update_list with the frame byte) per interval.

def _stream(W, H, n_slices, seed, extra=(), gap=None):
    """Background events over n_slices ms plus `extra` (x, y, t) events; gap = (t0, t1): no events in [t0, t1)."""
    from nsof import synth
    dur = n_slices * 1000
    x, y, p, t = synth.make_events(seed, W, H, max(2000, W * H // 40), dur, box=(min(20, W // 4), min(16, H // 4)))
    if gap is not None:
        keep = (t < gap[0]) | (t >= gap[1])
        x, y, p, t = x[keep], y[keep], p[keep], t[keep]
    xs, ys, ts = [x], [y], [t]
    for (ex, ey, et) in extra:
        xs.append(np.asarray(ex, np.int16))
        ys.append(np.asarray(ey, np.int16))
        ts.append(np.asarray(et, np.int64))
    x, y, t = np.concatenate(xs), np.concatenate(ys), np.concatenate(ts)
    o = np.argsort(t, kind="stable")
    return x[o].astype(np.int16), y[o].astype(np.int16), np.ones(o.size, np.int8), t[o]


def _frames_case(nsof_lib, ctx, oracle, torch_dev, H, W, every, n_frames, x, y, t, view="dense", mode="state"):
    """run_frames on the default path, on dense=True (n x run_surface) and against the oracle: same frames, same state."""
    import torch
    from nsof.accumulator import Accumulator, slice_index_array
    idx = slice_index_array(t, 1000)
    assert len(idx) - 1 >= n_frames * every
    want, w_ref, band = _ref_frames(oracle, x, y, idx, H, W, 0, n_frames, every, -6.0, 0.0, mode)
    assert band == 0
    got = {}
    for dense in (None, True):
        acc = Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx, dense=dense)
        try:
            acc.set_events(x, y, p_ones(t), t, idx)
            if view == "dense":
                frames = torch.zeros((n_frames, H, W), dtype=torch.uint8, device=torch_dev)
            elif view == "row16":          # rows padded to a multiple of 16: still 16-byte addressable
                frames = torch.zeros((n_frames, H, W + 16), dtype=torch.uint8, device=torch_dev)[:, :, :W]
            elif view == "row4":           # a row stride that is not a multiple of 16
                frames = torch.zeros((n_frames, H, W + 4), dtype=torch.uint8, device=torch_dev)[:, :, :W]
            elif view == "offset1":        # the frames' base one byte past a 16-byte boundary
                flat = torch.zeros(n_frames * H * W + 16, dtype=torch.uint8, device=torch_dev)
                frames = flat[1:1 + n_frames * H * W].view(n_frames, H, W)
            torch.cuda.synchronize()
            acc.run_frames(0, n_frames, every, frames, mode=mode)
            ctx.synchronize()
            got[dense] = (frames.cpu().numpy(), acc.w())
        finally:
            acc.close()
    assert np.array_equal(got[None][0], want)
    assert np.array_equal(got[True][0], want)
    assert _same(got[None][1], w_ref) and _same(got[True][1], w_ref)
    return want


def p_ones(t):
    return np.ones(len(t), np.int8)


@pytest.mark.parametrize("every,n_frames", [(1, 131), (2, 65)])
def test_run_frames_tile_walk_many_intervals(nsof_lib, ctx, oracle, torch_dev, every, n_frames):
    """Tile walk (W = 160): more than 63 intervals, so k_tile_frames takes its chunks of 63 intervals more than once; the
    last chunk holds 5 / 2 intervals, not a multiple of its prefetch depth (4)."""
    H, W = 48, 160
    x, y, _, t = _stream(W, H, every * n_frames + 2, 41)
    _frames_case(nsof_lib, ctx, oracle, torch_dev, H, W, every, n_frames, x, y, t)


def test_run_frames_tile_walk_two_frames(nsof_lib, ctx, oracle, torch_dev):
    """Tile walk with n_frames = 2, the fewest it takes."""
    H, W = 64, 96
    x, y, _, t = _stream(W, H, 80, 42)
    _frames_case(nsof_lib, ctx, oracle, torch_dev, H, W, 33, 2, x, y, t)


@pytest.mark.parametrize("H,W", [(1024, 1024), (1025, 1024), (1280, 1024), (77, 208)])
def test_run_frames_tile_walk_tile_counts(nsof_lib, ctx, oracle, torch_dev, H, W):
    """Tile walk at exactly 1024 tiles, 1025 and 1280 (the bucket scan then gives each thread more than one tile), and a
    pixel count that is not a multiple of 1024 (77 x 208: the last tile ends inside the image)."""
    x, y, _, t = _stream(W, H, 62, 43)
    _frames_case(nsof_lib, ctx, oracle, torch_dev, H, W, 20, 3, x, y, t)


def test_run_frames_tile_walk_64_slice_intervals(nsof_lib, ctx, oracle, torch_dev):
    """Tile walk, every = 64 (records carry the slice in 6 bits): events in slice 63 of an interval, one pixel with an
    event in every slice of an interval, events at pixel 0 and at npx - 1."""
    H, W = 50, 112
    ts = np.arange(64, 128) * 1000 + 500                            # pixel (7, 5): every slice of interval 1
    extra = [(np.full(64, 7), np.full(64, 5), ts),
             ([0, 0, W - 1, W - 1], [0, 0, H - 1, H - 1], [63_100, 191_900, 100, 127_999]),
             (np.arange(10), np.full(10, 9), np.full(10, 63_700))]    # slice 63 of interval 0
    x, y, _, t = _stream(W, H, 3 * 64 + 1, 44, extra)
    from nsof.accumulator import slice_index_array
    idx = slice_index_array(t, 1000)
    assert idx[64] > idx[63] and idx[128] > idx[127]
    _frames_case(nsof_lib, ctx, oracle, torch_dev, H, W, 64, 3, x, y, t)


@pytest.mark.parametrize("view", ["dense", "row16"])
def test_run_frames_tile_walk_empty_intervals(nsof_lib, ctx, oracle, torch_dev, view):
    """Tile walk over intervals without any event (a gap of 5 intervals), dense frames and 16-byte-aligned strided views."""
    H, W = 40, 96
    x, y, _, t = _stream(W, H, 10 * 10, 45, gap=(30_000, 80_000))
    _frames_case(nsof_lib, ctx, oracle, torch_dev, H, W, 10, 10, x, y, t, view=view, mode="state")


@pytest.mark.parametrize("view", ["row4", "offset1"])
def test_run_frames_copy_patch_views(nsof_lib, ctx, oracle, torch_dev, view):
    """Copy + patch: a row stride that is not a multiple of 16, or frames whose base is one byte off 16-byte alignment,
    fail tile_ok; empty intervals and the pixels 0 / npx - 1 on that path too."""
    H, W = 40, 96
    extra = [([0, W - 1], [0, H - 1], [5_500, 21_500])]
    x, y, _, t = _stream(W, H, 8 * 10, 46, extra, gap=(30_000, 60_000))
    _frames_case(nsof_lib, ctx, oracle, torch_dev, H, W, 10, 8, x, y, t, view=view)
