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
