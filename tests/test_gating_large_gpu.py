"""Device ROI gating of maps above 64 x 64 cells (nsof_roi_from_surface_dev's union-find path) against the host C mirror
(gating.roi_from_surface) and gating.current_to_gray, and the pipelines that gate on such maps: events_to_rois,
events_to_roi_flows and both sequence experiments.  Inputs come from seeds."""
import numpy as np
import pytest

SIZES = [(65, 65), (64, 65), (65, 64), (1, 5000), (5000, 1), (90, 160), (108, 192), (256, 256), (257, 256), (540, 960)]
DENSITIES = (0.3, 0.45, 0.55, 0.6)


def _snake(rows, cols):
    on = np.zeros((rows, cols), bool)
    on[::2, :] = True
    for r in range(1, rows, 2):
        on[r, (cols - 1) if (r // 2) % 2 == 0 else 0] = True
    return on


def _spiral(rows, cols):
    on = np.zeros((rows, cols), bool)
    top, left, bottom, right = 0, 0, rows - 1, cols - 1
    while top <= bottom and left <= right:
        on[top, left:right + 1] = True
        on[top:bottom + 1, right] = True
        if bottom - top >= 2:
            on[bottom, left:right + 1] = True
        if right - left >= 2 and bottom - top >= 4:
            on[top + 2:bottom + 1, left] = True
            if left + 2 <= right:
                on[top + 2, left:left + 3] = True
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return on


def _comb(rows, cols):
    on = np.zeros((rows, cols), bool)
    on[:, ::2] = True              # teeth hanging from the top, joined only by the last row
    on[-1, :] = True
    return on


def _maps(rng, rows, cols):
    """Random maps near percolation plus the adversarial ones, as ON masks."""
    maps = [rng.random((rows, cols)) < d for d in DENSITIES]
    maps.append((np.add.outer(np.arange(rows), np.arange(cols)) % 2) == 0)     # checkerboard
    maps.append(np.zeros((rows, cols), bool))
    maps.append(np.ones((rows, cols), bool))
    last = np.zeros((rows, cols), bool)
    last[-1, -1] = True
    maps.append(last)
    if rows >= 4 and cols >= 4:
        maps += [_snake(rows, cols), _spiral(rows, cols), _comb(rows, cols)]
    return maps


def _currents(rng, on):
    """Device currents whose gray values cross THRES 200 exactly where `on` is set; a few cells <= 0 (gray 0: NaN path)."""
    cur = np.where(on, 10.0 ** rng.uniform(-6.6, -4.0, on.shape), 10.0 ** rng.uniform(-12.0, -7.0, on.shape))
    off = ~on
    if off.any():
        idx = np.flatnonzero(off)
        pick = rng.choice(idx, size=min(3, idx.size), replace=False)
        cur.flat[pick[: len(pick) // 2 + 1]] = 0.0
        cur.flat[pick[len(pick) // 2 + 1:]] = -1.0
    return cur


def _cfg(gating, flag, conn, ms):
    return gating.GatingConfig(MEMSIZE=ms, THRES=200, FLAG=flag, CONNECT=conn, EXTEND_HEIGHT_UPPER=2, EXTEND_HEIGHT_LOWER=3,
                               EXTEND_WIDTH_LEFT=1, EXTEND_WIDTH_RIGHT=4)


def _upload(torch, dev, curs, pad):
    """Maps k at + k * (rows * cols + pad) doubles."""
    n, cells = len(curs), curs[0].size
    buf = np.full((n, cells + pad), np.nan)
    for k, c in enumerate(curs):
        buf[k, :cells] = c.ravel()
    d = torch.from_numpy(buf).to(dev)
    torch.cuda.synchronize()
    return d, cells + pad


@pytest.mark.gpu
@pytest.mark.parametrize("rows,cols", SIZES)
def test_large_maps_equal_host_mirror(nsof_lib, ctx, rows, cols):
    """Every FLAG x CONNECT setting: rectangle lists equal the host mirror's in order, gray maps byte-identical, counts true
    even when the table is smaller (max_rects 1 and true count - 1: the stored prefix is the mirror's)."""
    import torch
    from nsof import gating
    rng = np.random.default_rng(rows * 7919 + cols)
    dev = torch.device("cuda", ctx.device)
    ms = 3
    h, w = rows * ms + 2, cols * ms + 5
    curs = [_currents(rng, on) for on in _maps(rng, rows, cols)]
    n = len(curs)
    d, stride = _upload(torch, dev, curs, pad=17)
    for flag in (1, 2):
        for conn in (4, 8):
            cfg = _cfg(gating, flag, conn, ms)
            want = [gating.roi_from_surface(c, (h, w), cfg) for c in curs]
            cap = max(1, max(len(v) for v in want))
            counts, rects, gray = gating.roi_from_surface_dev(d, n, (rows, cols), (h, w), cfg, max_rects=cap, ctx=ctx,
                                                              want_gray=True, map_stride=stride)
            got = gating.rects_to_host(counts, rects, ctx=ctx)
            for k in range(n):
                assert got[k] == want[k], (rows, cols, flag, conn, k, got[k][:4], want[k][:4])
            if flag == 1 and conn == 4:
                g = gray.cpu().numpy()
                for k in range(n):
                    assert np.array_equal(g[k], gating.current_to_gray(curs[k])), (rows, cols, k)
            if flag == 1:
                true = [len(v) for v in want]
                for small in sorted({1, max(1, cap - 1)}):
                    c2, r2 = gating.roi_from_surface_dev(d, n, (rows, cols), (h, w), cfg, max_rects=small, ctx=ctx,
                                                         map_stride=stride)
                    ctx.synchronize()
                    assert c2.cpu().numpy().tolist() == true, (rows, cols, conn, small)
                    r2 = r2.cpu().numpy()
                    for k in range(n):
                        m = min(true[k], small)
                        assert [tuple(int(q) for q in r2[k, i]) for i in range(m)] == want[k][:m], (rows, cols, conn, small, k)
    # component counts of the adversarial maps are what they are built to be
    if rows >= 4 and cols >= 4:
        cfg = _cfg(gating, 1, 4, ms)
        cb = gating.roi_from_surface(curs[len(DENSITIES)], (h, w), cfg)
        assert len(cb) == (rows * cols + 1) // 2
        assert len(gating.roi_from_surface(curs[len(DENSITIES)], (h, w), _cfg(gating, 1, 8, ms))) == 1
        assert [len(gating.roi_from_surface(c, (h, w), cfg)) for c in curs[-3:]] == [1, 1, 1]   # snake, spiral, comb


@pytest.mark.gpu
def test_large_map_gating_is_deterministic(nsof_lib, ctx):
    """The same batch of near-percolation 540 x 960 maps gated twice gives identical tables (and the mirror's): counts and
    every stored rectangle (rows past a map's count are not written)."""
    import torch
    from nsof import gating
    rng = np.random.default_rng(11)
    dev = torch.device("cuda", ctx.device)
    rows, cols, ms = 540, 960, 4
    h, w = rows * ms, cols * ms
    curs = [_currents(rng, rng.random((rows, cols)) < d) for d in (0.55, 0.6, 0.59, 0.45, 0.62, 0.58)]
    d, stride = _upload(torch, dev, curs, pad=0)
    for conn in (4, 8):
        cfg = _cfg(gating, 1, conn, ms)
        want = [gating.roi_from_surface(c, (h, w), cfg) for c in curs]
        cap = max(len(v) for v in want)
        a = gating.roi_from_surface_dev(d, len(curs), (rows, cols), (h, w), cfg, max_rects=cap, ctx=ctx)
        b = gating.roi_from_surface_dev(d, len(curs), (rows, cols), (h, w), cfg, max_rects=cap, ctx=ctx)
        ctx.synchronize()
        assert torch.equal(a[0], b[0]), conn
        ra, rb = a[1].cpu().numpy(), b[1].cpu().numpy()
        for k, c in enumerate(a[0].cpu().numpy().tolist()):
            assert np.array_equal(ra[k, :c], rb[k, :c]), (conn, k)
        assert gating.rects_to_host(*a, ctx=ctx) == want, conn


# ---- more maps than one chunk ---------------------------------------------------------------------------------------------
# nsof_roi_from_surface_dev labels maps above 64 x 64 cells a chunk of maps at a time (csrc/gating_kernels.hip).  The mirror
# of its chunk arithmetic: tiles of CCL_TILE = 256 cells; FLAG 1 needs 4 bytes per cell and per tile of workspace; a
# chunk is at most 2^23 tiles, and at most what the context's workspace holds, taken as at least 64 MiB.
CCL_TILE = 256
MAX_CHUNK_TILES = 1 << 23
WORKSPACE_FLOOR = 64 << 20
CHUNK_ROWS, CHUNK_COLS = 128, 130


def _chunk_maps(rows, cols, workspace_bytes=0):
    """Maps per chunk of a FLAG 1 call on a context whose workspace holds `workspace_bytes` (a fresh one: 0)."""
    ncell = rows * cols
    ntile = -(-ncell // CCL_TILE)
    per_map = 4 * (ncell + ntile)
    return min(max(1, MAX_CHUNK_TILES // ntile), max(1, max(workspace_bytes, WORKSPACE_FLOOR) // per_map))


def _n_maps_for_three_chunks():
    return 2 * _chunk_maps(CHUNK_ROWS, CHUNK_COLS) + 3


def test_chunk_arithmetic_of_the_many_maps_case():
    """128 x 130 cells: 16640 cells in 65 tiles, 66820 bytes per map, 1004 maps per chunk on a fresh context -- 2011 maps
    are two full chunks and a tail of three.  (The constants are read back from the source, so that the mirror above
    cannot fall behind them unnoticed.)"""
    import os
    import re
    from conftest import PKG
    with open(os.path.join(PKG, "csrc", "gating_kernels.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int CCL_TILE = (\d+);", src).group(1)) == CCL_TILE
    assert "((size_t)1 << 23) / ntile" in src and "(size_t)64 << 20" in src
    assert CHUNK_ROWS > 64 and CHUNK_COLS > 64                      # the union-find path, not one wavefront per map
    assert 4 * (128 * 130 + 65) == 66820
    chunk = _chunk_maps(CHUNK_ROWS, CHUNK_COLS)
    assert chunk == min(2 ** 23 // 65, 2 ** 26 // 66820) == 1004
    n_maps = _n_maps_for_three_chunks()
    assert n_maps == 2011 and n_maps > 2 * chunk and n_maps - 2 * chunk == 3
    assert _chunk_maps(CHUNK_ROWS, CHUNK_COLS, 1 << 30) >= n_maps   # a context with a 1 GiB workspace takes one pass


def _sparse_currents(n_maps, rows, cols, pad):
    """`n_maps` sparse maps, each from its own seed, as device currents in one buffer [n_maps][rows * cols + pad] (the pad
    NaN) -> (buffer, ON masks).  A map has 1..20 blobs: up to three diagonal chains of 2..4 cells (one component under
    CONNECT 8, one per cell under CONNECT 4) and small rectangles otherwise -- at most 3 * 4 + 17 components, within a
    table of 32.  ON / OFF currents as `_currents` draws them; up to three OFF cells are 0 or negative."""
    cells = rows * cols
    buf = np.full((n_maps, cells + pad), np.nan)
    ons = np.zeros((n_maps, rows, cols), bool)
    for k in range(n_maps):
        rng = np.random.default_rng(500_000 + k)
        on = ons[k]
        blobs = int(rng.integers(1, 21))
        chains = min(blobs, int(rng.integers(0, 4)))
        for _ in range(chains):
            n, step = int(rng.integers(2, 5)), int(rng.choice((-1, 1)))
            r0, c0 = int(rng.integers(0, rows - 4)), int(rng.integers(4, cols - 4))
            on[r0 + np.arange(n), c0 + step * np.arange(n)] = True
        for _ in range(blobs - chains):
            r0, c0 = int(rng.integers(0, rows)), int(rng.integers(0, cols))
            on[r0:r0 + int(rng.integers(1, 7)), c0:c0 + int(rng.integers(1, 9))] = True
        cur = 10.0 ** np.where(on, rng.uniform(-6.6, -4.0, on.shape), rng.uniform(-12.0, -7.0, on.shape))
        pick = rng.integers(0, cells, 3)
        pick = pick[~on.flat[pick]]
        cur.flat[pick[:2]] = 0.0
        cur.flat[pick[2:]] = -1.0
        buf[k, :cells] = cur.ravel()
    return buf, ons


@pytest.mark.gpu
def test_more_maps_than_one_chunk(nsof_lib, ctx):
    """2011 maps of 128 x 130 cells in one call on a fresh context: the chunk loop of nsof_roi_from_surface_dev runs three
    times (1004 + 1004 + 3 maps, `_chunk_maps`), each time from offsets into the currents, the counts, the rectangle
    table and the gray maps.  Every map's rectangles equal the host mirror's and its gray map current_to_gray, for CONNECT
    4 and 8; the shared context (whose workspace, and so whose chunking, is whatever earlier calls left) and the fresh
    context a second time (its workspace now reserved) give the same tables.  FLAG 2 on the same batch equals its
    mirror too, but in a single pass: it needs no workspace, and its own chunk of 2^23 // 65 maps is out of a test's
    reach."""
    import torch
    from nsof import gating
    rows, cols, ms, pad, cap = CHUNK_ROWS, CHUNK_COLS, 3, 17, 32
    chunk = _chunk_maps(rows, cols)
    n_maps = _n_maps_for_three_chunks()
    assert n_maps > 2 * chunk and rows > 64
    h, w = rows * ms + 2, cols * ms + 5
    buf, ons = _sparse_currents(n_maps, rows, cols, pad)
    curs = buf[:, :rows * cols].reshape(n_maps, rows, cols)
    assert (curs <= 0).any(axis=(1, 2)).sum() > n_maps // 2          # cells of gray 0 through the NaN path
    for k in range(n_maps):                                           # a map read at another chunk's offset is another map
        for other in (k + chunk, k + 2 * chunk):
            assert other >= n_maps or not np.array_equal(ons[k], ons[other]), (k, other)
    gray_ref = gating.current_to_gray(curs)
    assert np.array_equal(gray_ref >= 200, ons)
    dev = torch.device("cuda", ctx.device)
    d = torch.from_numpy(buf).to(dev)
    torch.cuda.synchronize()
    stride = rows * cols + pad
    fresh = nsof_lib.Context(0)
    try:
        want = {}
        for conn in (4, 8):
            cfg = _cfg(gating, 1, conn, ms)
            want[conn] = [gating.roi_from_surface(c, (h, w), cfg) for c in curs]
            n_rects = [len(v) for v in want[conn]]
            assert 1 <= min(n_rects) and max(n_rects) <= cap, (conn, min(n_rects), max(n_rects))
            for m0 in range(0, n_maps, chunk):                        # a count written at another map's slot shows
                assert len(set(n_rects[m0:m0 + chunk])) >= 2, (conn, m0)
            counts, rects, gray = gating.roi_from_surface_dev(d, n_maps, (rows, cols), (h, w), cfg, max_rects=cap, ctx=fresh,
                                                              want_gray=True, map_stride=stride)
            got = gating.rects_to_host(counts, rects, ctx=fresh)
            for k in range(n_maps):
                assert got[k] == want[conn][k], (conn, k, k // chunk, got[k][:4], want[conn][k][:4])
            g = gray.cpu().numpy()
            for k in range(n_maps):
                assert np.array_equal(g[k], gray_ref[k]), (conn, k, k // chunk)
            # FLAG 2: one pass over the whole batch
            cfg2 = _cfg(gating, 2, conn, ms)
            c2, r2 = gating.roi_from_surface_dev(d, n_maps, (rows, cols), (h, w), cfg2, max_rects=cap, ctx=fresh,
                                                 map_stride=stride)
            got2 = gating.rects_to_host(c2, r2, ctx=fresh)
            for k in range(n_maps):
                assert got2[k] == gating.roi_from_surface(curs[k], (h, w), cfg2), (conn, k)
            # the shared context, then the fresh one again: counts and every stored rectangle are the same
            c_ref, r_ref = counts.cpu().numpy(), rects.cpu().numpy()
            stored = np.arange(cap)[None, :] < c_ref[:, None]
            for which in (ctx, fresh):
                c3, r3 = gating.roi_from_surface_dev(d, n_maps, (rows, cols), (h, w), cfg, max_rects=cap, ctx=which,
                                                     map_stride=stride)
                which.synchronize()
                assert np.array_equal(c3.cpu().numpy(), c_ref), (conn, which is ctx)
                assert np.array_equal(r3.cpu().numpy()[stored], r_ref[stored]), (conn, which is ctx)
        assert sum(a != b for a, b in zip(want[4], want[8])) > n_maps // 4   # the chains: CONNECT 4 and 8 differ
    finally:
        fresh.close()


def _union(rects):
    return [(min(r[0] for r in rects), min(r[1] for r in rects), max(r[2] for r in rects), max(r[3] for r in rects))] if rects else []


@pytest.mark.gpu
def test_events_to_rois_takes_the_device_path_for_a_90x160_map(nsof_lib, ctx, monkeypatch):
    """A 1280 x 720 stream at MEMSIZE 8 (90 x 160 cells) gates on the device: the host mirror is not called, and what comes
    back equals the real events_to_rois_host."""
    from nsof import gating, pipeline, synth
    H, W = 720, 1280   # noqa: N806
    x, y, p, t = synth.make_events(17, W, H, n_background=20_000, duration_us=120_000, box=(160, 100), speed_pps=600.0)
    real_host = pipeline.events_to_rois_host

    def refuse(*a, **kw):
        raise AssertionError("events_to_rois fell back to the host gating mirror")

    monkeypatch.setattr(pipeline, "events_to_rois_host", refuse)
    for flag in (1, 2):
        cfg = gating.GatingConfig(MEMSIZE=8, EXTEND_HEIGHT_UPPER=6, EXTEND_HEIGHT_LOWER=6, EXTEND_WIDTH_LEFT=6,
                                  EXTEND_WIDTH_RIGHT=6, THRES=240, FLAG=flag)
        a = pipeline.events_to_rois(x, y, p, t, (H, W), cfg, slice_us=1000, silent_v=0.5, snapshot_every=30, ctx=ctx)
        b = real_host(x, y, p, t, (H, W), cfg, slice_us=1000, silent_v=0.5, snapshot_every=30, ctx=ctx)
        assert len(a) == len(b) == 4 and a[0][0].shape == (90, 160)
        for (ga, ra), (gb, rb) in zip(a, b):
            assert np.array_equal(ga, gb)
            assert ra == (rb if flag == 1 else _union(rb))
        if flag == 1:
            assert max(len(r) for _, r in a) > 32      # the table was regrown


@pytest.mark.gpu
@pytest.mark.parametrize("bug_compatible", [True, False])
def test_events_to_roi_flows_with_a_72x128_map(nsof_lib, ctx, oracle, bug_compatible):
    """events_to_roi_flows on a 640 x 360 stream at MEMSIZE 5 (72 x 128 cells) against the chain: oracle accumulator ->
    block currents -> host gating mirror -> GPU Farneback of every crop (farneback_pairs), pasted in label order."""
    from nsof import gating, pipeline, synth
    from nsof.farneback import PARAMS_B, farneback_pairs
    H, W, every, ms = 360, 640, 40, 5   # noqa: N806
    x, y, p, t = synth.make_events(9, W, H, n_background=2500, duration_us=160_000, box=(80, 60), speed_pps=500.0)
    ref_frames, ref_cur = [], []
    for k in range(4):
        _, wst = oracle.accum_slices_per_s(x, y, t, H, W, 1000, -6.0, 0.5, n_slices=(k + 1) * every, n_threads=4)
        ref_frames.append((np.float32(255.0) * wst).astype(np.uint8))
        ref_cur.append(pipeline.surface_to_block_current(oracle.accum_resistance(wst), ms))
    assert ref_cur[0].shape == (72, 128)
    gi = 0 if bug_compatible else 1
    for flag in (1, 2):
        cfg = gating.GatingConfig(MEMSIZE=ms, EXTEND_HEIGHT_UPPER=10, EXTEND_HEIGHT_LOWER=10, EXTEND_WIDTH_LEFT=10,
                                  EXTEND_WIDTH_RIGHT=10, THRES=240, FLAG=flag, farneback_params=PARAMS_B,
                                  bug_compatible=bug_compatible)
        frames, rects, flows = pipeline.events_to_roi_flows(x, y, p, t, (H, W), cfg, slice_us=1000, silent_v=0.5,
                                                            snapshot_every=every, ctx=ctx)
        gf, gfl = frames.cpu().numpy(), flows.cpu().numpy()
        assert gf.shape == (4, H, W) and gfl.shape == (3, H, W, 2)
        for k in range(4):
            assert np.array_equal(gf[k], ref_frames[k]), k
            assert rects[k] == gating.roi_from_surface(ref_cur[k], (H, W), cfg), (flag, k)
        for k in range(3):
            rs = rects[k + gi]
            crops = [(np.ascontiguousarray(gf[k][y0:y1, x0:x1]), np.ascontiguousarray(gf[k + 1][y0:y1, x0:x1]))
                     for (x0, y0, x1, y1) in rs]
            canvas = np.zeros((H, W, 2), np.float32)
            for (x0, y0, x1, y1), f in zip(rs, farneback_pairs(crops, PARAMS_B, ctx=ctx) if crops else []):
                canvas[y0:y1, x0:x1] = f
            assert np.array_equal(gfl[k], canvas), (flag, bug_compatible, k)
        assert any(len(r) for r in rects[1:])
        if flag == 1:
            assert max(len(r) for r in rects) > 1


def _blob_stack(seed, rows, cols, n, noise):
    """A 'constructed3DMatrix' stack [rows][cols][n]: an ON blob moving right plus isolated ON noise cells."""
    rng = np.random.default_rng(seed)
    st = 10.0 ** rng.uniform(-12.0, -7.5, (rows, cols, n))
    for s in range(n):
        r0, c0 = rows // 3, 4 + 5 * s
        st[r0:r0 + rows // 3, c0:c0 + 9, s] = 2e-5
        on = rng.random((rows, cols)) < noise
        st[:, :, s][on] = 3e-6
    return st


def _synthetic_bgr(seed, n, h, w):
    from nsof import workload as wl
    return [np.ascontiguousarray(np.repeat(f[..., None], 3, 2)) for f in wl.synthetic_sequence(seed, n, h, w)]


LARGE = dict(MEMSIZE=8, EXTEND_HEIGHT_UPPER=8, EXTEND_HEIGHT_LOWER=8, EXTEND_WIDTH_LEFT=8, EXTEND_WIDTH_RIGHT=8, THRES=240)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [1, 2])
def test_prediction_sequence_dev_with_a_20x70_map(nsof_lib, ctx, torch_dev, flag):
    """prediction_sequence_dev == run_prediction (GPU backends), bit for bit, on a gating grid 70 cells wide; with FLAG 1
    the maps have more components than max_rects=32, so the table is regrown."""
    import torch
    from nsof import pipeline, predict
    rows, cols, n = 20, 70, 5
    h, w = rows * LARGE["MEMSIZE"], cols * LARGE["MEMSIZE"]
    stack = _blob_stack(41, rows, cols, n, 0.04 if flag == 1 else 0.01)
    frames = _synthetic_bgr(42, n, h, w)
    kw = dict(LARGE, FLAG=flag)
    preds = []

    def rec(*a, **k):
        out = predict.task_results(*a, **k, ctx=ctx)
        preds.append(out)
        return out

    fl = lambda a, b, f, **k: nsof_lib.calcOpticalFlowFarneback(a, b, f, **k, ctx=ctx)  # noqa: E731
    ssim = lambda p, t: predict.calculateIntegralError(p, t, ctx=ctx)  # noqa: E731
    rows_h, s_mem, s_orig, _, _ = pipeline.run_prediction(frames, stack, nsof_lib.dataset_config("grasp", **kw), flow_fn=fl,
                                                          predict_fn=rec, ssim_fn=ssim)
    d = torch.from_numpy(np.stack(frames)).to(torch_dev)
    torch.cuda.synchronize()
    res = pipeline.prediction_sequence_dev(d, stack, nsof_lib.dataset_config("grasp", **kw), ctx=ctx)
    pm, po = res["pred_mem"].cpu().numpy(), res["pred_orig"].cpu().numpy()
    sm, so = res["ssim_mem"].cpu().numpy(), res["ssim_orig"].cpu().numpy()
    assert len(rows_h) == n - 2
    for k in range(n - 2):
        assert np.array_equal(pm[k], preds[2 * k]), (flag, k, "mem")
        assert np.array_equal(po[k], preds[2 * k + 1]), (flag, k, "orig")
        assert sm[k] == s_mem[k] and so[k] == s_orig[k], (flag, k)
    if flag == 1:
        assert max(len(r) for r in res["rects"]) > 32


@pytest.mark.gpu
@pytest.mark.parametrize("flag", [1, 2])
def test_segmentation_sequence_dev_with_a_20x70_map(nsof_lib, ctx, torch_dev, flag):
    """segmentation_sequence_dev == run_segmentation (GPU backends), bit for bit, on the same 70-cell-wide grid."""
    import torch
    from nsof import gating, pipeline, segment
    rows, cols, n = 20, 70, 5
    h, w = rows * LARGE["MEMSIZE"], cols * LARGE["MEMSIZE"]
    stack = _blob_stack(51, rows, cols, n, 0.04 if flag == 1 else 0.01)
    frames = _synthetic_bgr(52, n, h, w)
    rng = np.random.default_rng(53)
    gts = [rng.integers(100, 156, (h, w, 3), dtype=np.uint8) for _ in range(n)]
    for g in gts:
        g[h // 4:h // 2, w // 3:w // 2] = 255
    kw = dict(LARGE, FLAG=flag)
    masks = []

    def rec(f):
        out = segment.motion_mask(f, 1, ctx=ctx)
        masks.append(out.copy())
        return out

    fl = lambda a, b, f, **k: nsof_lib.calcOpticalFlowFarneback(a, b, f, **k, ctx=ctx)  # noqa: E731
    rows_h, m_mem, m_orig = pipeline.run_segmentation(frames, gts, stack, nsof_lib.dataset_config("grasp", **kw), flow_fn=fl,
                                                      mask_fn=rec)
    d = torch.from_numpy(np.stack(frames)).to(torch_dev)
    g = torch.from_numpy(np.stack(gts)).to(torch_dev)
    torch.cuda.synchronize()
    res = pipeline.segmentation_sequence_dev(d, g, stack, nsof_lib.dataset_config("grasp", **kw), ctx=ctx)
    mm, mo = res["mask_mem"].cpu().numpy(), res["mask_orig"].cpu().numpy()
    pm, po = res["pa_mem"].cpu().numpy(), res["pa_orig"].cpu().numpy()
    assert len(rows_h) == n - 2
    it = iter(masks)
    for k in range(n - 2):
        want = np.zeros((h, w), np.uint8)
        for x0, y0, x1, y1 in res["boxes"][k]:
            if x1 > x0 and y1 > y0:
                want[y0:y1, x0:x1] = next(it)
        assert np.array_equal(mm[k], want), (flag, k, "mem")
        assert np.array_equal(mo[k], next(it)), (flag, k, "orig")
        gt = np.where(gating.frame_to_gray(gts[k + 1], "BGR2GRAY") > 127, np.uint8(255), np.uint8(0))
        assert pm[k] == pipeline.calculate_pixel_accuracy(mm[k], gt), (flag, k)
        assert po[k] == pipeline.calculate_pixel_accuracy(mo[k], gt), (flag, k)
    assert next(it, None) is None
    assert res["mean_mem"] == m_mem and res["mean_orig"] == m_orig
    if flag == 1:
        assert max(len(r) for r in res["rects"]) > 32
