"""The prediction experiment of optical_flow_prediction.py (__main__ :435-681, task_results :257-361) over a sequence.

CPU: ``pipeline.run_prediction`` (the script's loop, CSV schema and formatting, SSIM against frame i+2, the printed
means that divide by cnt - 1) with the CPU oracle as flow / warp / SSIM backend, and the harness's box arithmetic
against the boxes ``predict.task_results`` warps.
GPU: the batched prediction warp (``nsof_predict_sequence_u8_dev``) against the per-box ``nsof_predict_warp_u8_dev``
composition and the oracle, the batched SSIM (``nsof_ssim_u8_batch_dev``) against the single-pair entry, the oracle and
scikit-image, and ``pipeline.prediction_sequence_dev`` against ``run_prediction`` with the GPU backends.
"""
import csv
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

from conftest import GOLDEN, golden_path

SMALL = dict(MEMSIZE=16, EXTEND_HEIGHT_UPPER=4, EXTEND_HEIGHT_LOWER=4, EXTEND_WIDTH_LEFT=4, EXTEND_WIDTH_RIGHT=4)


def _grasp_json_stack(keys=("0", "1", "2", "3")):
    g = json.load(open(golden_path("gating_maps.json")))["grasp"]
    return np.stack([np.array([[float(v) for v in row] for row in g["slices"][k]]) for k in keys], -1)


def _oracle_task(oracle):
    """``task_results`` restated on the CPU oracle (oracle.flow_map + oracle.remap_linear), box arithmetic written out
    as prediction.py:268-353 has it."""
    def task(prev, nxt, flow, num_labels, regions, EST_FLAG=2, MERGE_FLAG=False, times=None, comb_times=None,  # noqa: N803
             borderMode=1):  # noqa: N803
        t0 = time.time()
        h, w = prev.shape[:2]
        out = nxt.copy()
        boxes = []
        if num_labels > 1:
            if EST_FLAG == 1 and MERGE_FLAG:
                boxes = [(max(0, min(r[0] for r in regions) - 20), max(0, min(r[1] for r in regions) - 20),
                          min(w, max(r[2] for r in regions) + 20), min(h, max(r[3] for r in regions) + 20))]
            else:
                boxes = list(regions) if EST_FLAG == 1 else [tuple(regions)]
        if comb_times is not None:
            comb_times.append(time.time() - t0)
        for x0, y0, x1, y1 in boxes:
            mx, my = oracle.flow_map(flow, (x0, y0, x1, y1), sign=1)
            out[y0:y1, x0:x1] = oracle.remap_linear(nxt, mx, my, border=borderMode)
        if times is not None:
            times.append(time.time() - t0)
        return out
    return task


def _synthetic_bgr(seed, n, h, w):
    from nsof import workload as wl
    return [np.ascontiguousarray(np.repeat(f[..., None], 3, 2)) for f in wl.synthetic_sequence(seed, n, h, w)]


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_run_prediction_rows_csv_and_means(nsof_lib, oracle, tmp_path):
    from nsof import pipeline
    stack = _grasp_json_stack()
    hm, wm = stack.shape[:2]
    cfg = nsof_lib.dataset_config("grasp", **SMALL)
    h, w = hm * 16, wm * 16
    frames = _synthetic_bgr(5, 4, h, w)
    frames[3][:, :, 2] = 255 - frames[3][:, :, 2]     # frame 3 differs from frame 2 in the SSIM channel
    far = lambda a, b, _f, **kw: oracle.farneback(a, b, **kw)  # noqa: E731
    seen = []

    def ssim(pred, true):
        seen.append((pred, true))
        return oracle.ssim_u8(true[:, :, 2], pred[:, :, 2])

    rows, s_mem, s_orig, m_mem, m_orig = pipeline.run_prediction(
        frames, stack, cfg, csv_path=str(tmp_path / "metrics_predict.csv"), flow_fn=far, predict_fn=_oracle_task(oracle),
        ssim_fn=ssim)
    assert pipeline.PREDICT_CSV_COLUMNS == [
        "Frame_Pair", "Original_Flow_Time", "Mem_Flow_Time", "Flow_Time_Improvement", "Flow_Time_Improvement_Percent",
        "Original_Pred_Time", "Mem_Pred_Time", "Combination_Time", "Original_SSIM", "Mem_SSIM", "Region_Percent",
        "Cal_Times", "Velocity_Times"]
    with open(tmp_path / "metrics_predict.csv") as fh:
        got = list(csv.reader(fh))
    assert got[0] == pipeline.PREDICT_CSV_COLUMNS and len(got) == 3 and len(rows) == 2
    assert [r[0] for r in got[1:]] == ["2.jpg-1.jpg", "3.jpg-2.jpg"]
    for r in got[1:]:
        assert len(r) == 13
        for col in (1, 2, 3, 5, 6, 7, 8, 9):
            assert len(r[col].split(".")[1]) == 4, (col, r[col])      # '%.4f'
        assert len(r[4].split(".")[1]) == 2                            # '%.2f'
        assert r[10].startswith("[") and r[10].endswith("]")           # str() of the region list
    # the SSIMs: mem then original prediction of each pair, both against frame i+2
    assert len(seen) == 4
    for i in range(2):
        (p_mem, t_mem), (p_orig, t_orig) = seen[2 * i], seen[2 * i + 1]
        assert t_mem is frames[i + 2] and t_orig is frames[i + 2]
        assert s_mem[i] == oracle.ssim_u8(frames[i + 2][:, :, 2], p_mem[:, :, 2])
        assert rows[i][9] == f"{s_mem[i]:.4f}" and rows[i][8] == f"{s_orig[i]:.4f}"
        # the original prediction: the full-frame flow, negated, remapped with BORDER_CONSTANT 0
        g0, g1 = (nsof_lib.frame_to_gray(frames[k], "RGB2GRAY") for k in (i, i + 1))
        fl = oracle.farneback(g0, g1, **cfg.farneback_params.as_kwargs())
        mx, my = oracle.flow_map(fl, (0, 0, w, h), sign=-1)
        assert np.array_equal(p_orig, oracle.remap_linear(frames[i + 1], mx, my, border=0))
    assert m_mem == sum(s_mem) / (2 - 1) and m_orig == sum(s_orig) / (2 - 1)   # the script's cnt - 1
    cfg3 = nsof_lib.dataset_config("grasp", **SMALL)
    rows3, s3, o3, m3, mo3 = pipeline.run_prediction(frames[:3], stack, cfg3, flow_fn=far,
                                                     predict_fn=_oracle_task(oracle), ssim_fn=ssim)
    assert len(rows3) == 1 and len(s3) == 1 and m3 is None and mo3 is None


def test_prediction_boxes_match_task_results(nsof_lib, monkeypatch):
    """The harness's box arithmetic (pad 20, clip to the frame) is the box list ``predict.task_results`` warps."""
    from nsof import pipeline, predict
    warped = []
    monkeypatch.setattr(predict, "predict_region",
                        lambda nxt, flow, box, out=None, **kw: warped.append(tuple(int(v) for v in box)) or out)
    h, w = 90, 130
    frame = np.zeros((h, w, 3), np.uint8)
    flow = np.zeros((h, w, 2), np.float32)
    cases = [([(30, 20, 60, 50)], 1), ([(5, 7, 40, 30), (100, 60, 128, 88)], 1), ([(0, 0, w, h)], 1),
             ([(10, 10, 20, 20), (12, 15, 70, 40), (50, 2, 60, 8)], 1), ([], 1), ((20, 30, 125, 80), 2),
             ((0, 0, 0, 0), 2)]
    for regions, flag in cases:
        num_labels = (len(regions) + 1) if flag == 1 else (1 if tuple(regions) == (0, 0, 0, 0) else 2)
        for merge in (True, False):
            warped.clear()
            predict.task_results(frame, frame, flow, num_labels, regions, EST_FLAG=flag, MERGE_FLAG=merge)
            assert warped == pipeline.prediction_boxes(regions, num_labels, flag, merge, (h, w)), (regions, flag, merge)
    assert pipeline.prediction_boxes([(5, 7, 40, 30), (100, 60, 128, 88)], 3, 1, True, (h, w)) == [(0, 0, 130, 90)]
    assert pipeline.prediction_boxes([(30, 25, 60, 50)], 2, 1, True, (h, w)) == [(10, 5, 80, 70)]


# ---------------------------------------------------------------------------------------------------------------- GPU
def _table(torch_dev, lists, max_rects):
    import torch
    counts = torch.tensor([len(r) for r in lists], dtype=torch.int32, device=torch_dev)
    rects = torch.zeros((len(lists), max_rects, 4), dtype=torch.int32)
    for k, rs in enumerate(lists):
        for i, r in enumerate(rs):
            rects[k, i] = torch.tensor(r)
    return counts, rects.to(torch_dev)


def _per_box(nsof_lib, ctx, frames, flows, boxes_per_pair):
    """The per-box composition: a copy of frame k+1, ``nsof_predict_warp_u8_dev`` on each box in turn."""
    import torch
    dense = frames.contiguous()
    n_pairs, h, w = flows.shape[:3]
    outs = []
    for k in range(n_pairs):
        out = dense[k + 1].clone()
        torch.cuda.synchronize()
        for box in boxes_per_pair[k]:
            nsof_lib.predict_region_dev(dense[k + 1], flows[k], out, h, w, box, ctx=ctx)
        ctx.synchronize()
        outs.append(out.cpu().numpy())
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("strided", [False, True])
def test_predict_sequence_equals_per_box_composition(nsof_lib, ctx, oracle, torch_dev, strided):
    import torch
    from nsof import pipeline, predict
    n, h, w = 6, 67, 133
    g = torch.Generator().manual_seed(11)
    big = torch.randint(0, 256, (n, h + 5, w + 7, 3), dtype=torch.uint8, generator=g)
    frames = big.to(torch_dev)[:, 2:2 + h, 3:3 + w] if strided else big[:, :h, :w].contiguous().to(torch_dev)
    assert frames.is_contiguous() != strided
    flows = torch.randn((n - 2, h, w, 2), generator=g) * 3.0
    flows[0, :5] = 80.0           # footprints far outside the frame: the border rule
    flows[1, :, :9] = -0.25       # exact quarter pixels
    flows = flows.to(torch_dev)
    # map k: overlapping boxes, boxes touching every edge, one map without boxes, one whole-frame box
    lists = [[(10, 5, 60, 40), (40, 20, 100, 60), (55, 30, 70, 45)],
             [(0, 0, 20, h), (w - 15, 0, w, 30), (0, h - 9, w, h), (0, 0, w, 4)],
             [],
             [(0, 0, w, h)],
             [(70, 40, 90, 50)],
             [(3, 3, 10, 10), (120, 60, 133, 67)]]
    counts, rects = _table(torch_dev, lists, 8)
    torch.cuda.synchronize()
    for gate_frame in (0, 1):
        pair_lists = [lists[k + gate_frame] for k in range(n - 2)]
        for flag, merge in ((1, False), (1, True), (2, False)):
            if flag == 2:   # FLAG 2 tables hold the union box or nothing
                pair_lists_f = [[(min(r[0] for r in rs), min(r[1] for r in rs), max(r[2] for r in rs), max(r[3] for r in rs))]
                                if rs else [] for rs in lists]
                c2, r2 = _table(torch_dev, pair_lists_f, 1)
                use = (c2, r2)
                pl = [pair_lists_f[k + gate_frame] for k in range(n - 2)]
            else:
                use, pl = (counts, rects), pair_lists
            boxes = [pipeline.prediction_boxes(rs, len(rs) + 1, 1, merge, (h, w)) if flag == 1 else
                     pipeline.prediction_boxes(rs[0] if rs else (0, 0, 0, 0), 2 if rs else 1, 2, merge, (h, w))
                     for rs in pl]
            torch.cuda.synchronize()
            got = predict.predict_sequence_dev(frames, flows, counts=use[0], rects=use[1], gate_frame=gate_frame,
                                               merge_padding=20 if merge else None, ctx=ctx)
            ctx.synchronize()
            want = _per_box(nsof_lib, ctx, frames, flows, boxes)
            fr = frames.cpu().numpy()
            for k in range(n - 2):
                assert np.array_equal(got[k].cpu().numpy(), want[k]), (gate_frame, flag, merge, k)
                if not pl[k]:
                    assert np.array_equal(want[k], fr[k + 1])        # no boxes: the frame itself
    # the full-frame baseline: BORDER_CONSTANT 0, against the CPU oracle
    got = predict.predict_sequence_dev(frames, flows, border_mode=predict.BORDER_CONSTANT, ctx=ctx)
    ctx.synchronize()
    fr, fl = frames.cpu().numpy(), flows.cpu().numpy()
    for k in range(n - 2):
        mx, my = oracle.flow_map(fl[k], (0, 0, w, h), sign=-1)
        assert np.array_equal(got[k].cpu().numpy(), oracle.remap_linear(fr[k + 1], mx, my, border=0)), k


def _ssim_single(ctx, a, b, k, channel):
    """``nsof_ssim_u8_dev`` of pair k (true = b, prediction = a, as calculateIntegralError passes them)."""
    out = C.c_double()
    h, w = a.shape[1:3]
    step = a.shape[3] if a.dim() == 4 else 1
    off = channel if a.dim() == 4 else 0
    rc = ctx._lib.nsof_ssim_u8_dev(ctx.ptr, b[k].data_ptr() + off, int(b.stride(1)), step, a[k].data_ptr() + off,
                                   int(a.stride(1)), step, w, h, 255.0, C.byref(out))
    ctx.check(rc, "ssim")
    return out.value


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(7, 7, 3), (37, 53, 3), (120, 161, 3), (29, 70)])
def test_ssim_batch_equals_single_pair(nsof_lib, ctx, oracle, torch_dev, shape):
    import torch
    from nsof import predict
    g = torch.Generator().manual_seed(3)
    n = 5
    a = torch.randint(0, 256, (n,) + shape, dtype=torch.uint8, generator=g)
    b = a.clone()
    b[1:] = torch.clamp(a[1:].int() + torch.randint(-40, 41, (n - 1,) + shape, generator=g), 0, 255).to(torch.uint8)
    b[3] = 17                                            # a flat image
    a, b = a.to(torch_dev), b.to(torch_dev)
    torch.cuda.synchronize()
    got = predict.ssim_batch_dev(a, b, ctx=ctx)
    ctx.synchronize()
    got = got.cpu().numpy()
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    for k in range(n):
        assert got[k] == _ssim_single(ctx, a, b, k, 2), k
        pa, pb = (an[k][..., 2], bn[k][..., 2]) if len(shape) == 3 else (an[k], bn[k])
        assert abs(got[k] - oracle.ssim_u8(pb, pa)) < 1e-12, k
    assert got[0] == 1.0 or abs(got[0] - 1.0) < 1e-12


@pytest.mark.gpu
def test_ssim_batch_matches_skimage_golden(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import predict
    gz = np.load(golden_path("ssim_golden.npz"))
    for name in ("small", "odd", "wide", "frame", "flat"):
        a, b = gz[name + "_a"], gz[name + "_b"]
        pred = torch.from_numpy(np.stack([b, a, b])).to(torch_dev)
        true = torch.from_numpy(np.stack([a, b, a])).to(torch_dev)
        torch.cuda.synchronize()
        got = predict.ssim_batch_dev(pred, true, ctx=ctx)
        ctx.synchronize()
        for v in got.cpu().numpy():
            assert abs(v - float(gz[name + "_ssim"])) < 1e-12, name


def _run_both(nsof_lib, ctx, torch_dev, frames, stack, cfg_kw, name, merge_flag):
    import torch
    from nsof import pipeline, predict
    preds = []

    def rec(*a, **kw):
        out = predict.task_results(*a, **kw, ctx=ctx)
        preds.append(out)
        return out

    cfg = nsof_lib.dataset_config(name, **cfg_kw)
    fl = lambda a, b, f, **kw: nsof_lib.calcOpticalFlowFarneback(a, b, f, **kw, ctx=ctx)  # noqa: E731
    ssim = lambda p, t: predict.calculateIntegralError(p, t, ctx=ctx)  # noqa: E731
    rows, s_mem, s_orig, _, _ = pipeline.run_prediction(frames, stack, cfg, merge_flag=merge_flag, flow_fn=fl,
                                                        predict_fn=rec, ssim_fn=ssim)
    d = torch.from_numpy(np.stack(frames)).to(torch_dev)
    torch.cuda.synchronize()
    res = pipeline.prediction_sequence_dev(d, stack, nsof_lib.dataset_config(name, **cfg_kw), merge_flag=merge_flag,
                                           ctx=ctx)
    pm, po = res["pred_mem"].cpu().numpy(), res["pred_orig"].cpu().numpy()
    sm, so = res["ssim_mem"].cpu().numpy(), res["ssim_orig"].cpu().numpy()
    n_pairs = len(frames) - 2
    assert len(rows) == n_pairs and pm.shape == (n_pairs,) + frames[0].shape
    for k in range(n_pairs):
        assert np.array_equal(pm[k], preds[2 * k]), (name, k, "mem")
        assert np.array_equal(po[k], preds[2 * k + 1]), (name, k, "orig")
        assert sm[k] == s_mem[k] and so[k] == s_orig[k], (name, k)
    return res, rows


@pytest.mark.gpu
@pytest.mark.parametrize("bug_compatible", [True, False])
def test_prediction_sequence_dev_equals_harness_1080p(nsof_lib, ctx, torch_dev, bug_compatible):
    from nsof import workload as wl
    with np.load(os.path.join(GOLDEN, "gating_stacks.npz")) as z:
        stack = z["grasp"]
    h, w = wl.DATASET_FRAMES["grasp"][:2]
    frames = _synthetic_bgr(21, 8, h, w)
    res, rows = _run_both(nsof_lib, ctx, torch_dev, frames, stack, dict(bug_compatible=bug_compatible), "grasp", True)
    assert [len(r) for r in res["rects"]] == [1] * 6
    assert res["boxes"] == res["rects"]               # FLAG 2: the union box of every pair's map is the warped box


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["autodriving", "uav", "uavnew2", "tabletennis"])
def test_prediction_sequence_dev_equals_harness_real_frames(nsof_lib, ctx, torch_dev, name):
    pil = pytest.importorskip("PIL.Image")
    d = os.path.join(GOLDEN, "frames", name)
    paths = [os.path.join(d, f) for f in sorted(os.listdir(d), key=lambda s: int(s.split(".")[0]))]
    frames = [np.ascontiguousarray(np.asarray(pil.open(p).convert("RGB"))[..., ::-1]) for p in paths]
    with np.load(os.path.join(GOLDEN, "gating_stacks.npz")) as z:
        stack = z[name]
    merges = (True, False) if nsof_lib.dataset_config(name).FLAG == 1 else (True,)
    for merge in merges:
        for bug in (True, False):
            _run_both(nsof_lib, ctx, torch_dev, frames, stack, dict(bug_compatible=bug), name, merge)


@pytest.mark.gpu
def test_bad_inputs_raise_and_launch_nothing(nsof_lib, torch_dev):
    import torch
    from nsof import _lib, pipeline, predict
    from nsof.errors import NsofError, NsofValueError
    c = nsof_lib.Context(0)
    try:
        c.prof_enable(_lib.K_REMAP, _lib.K_SSIM)
        fr = torch.zeros((4, 32, 40, 3), dtype=torch.uint8, device=torch_dev)
        fl = torch.zeros((3, 32, 40, 2), dtype=torch.float32, device=torch_dev)
        torch.cuda.synchronize()
        with pytest.raises(NsofValueError):
            predict.predict_sequence_dev(fr.float(), fl, ctx=c)
        with pytest.raises(NsofValueError):
            predict.predict_sequence_dev(fr, fl[:, :, :39], ctx=c)
        with pytest.raises(NsofValueError):
            predict.predict_sequence_dev(fr[:3], fl, ctx=c)                  # 3 pairs need 4 frames
        with pytest.raises(NsofValueError):
            predict.ssim_batch_dev(fr.float(), fr.float(), ctx=c)
        with pytest.raises(NsofValueError):
            predict.ssim_batch_dev(fr[:, :, :6], fr[:, :, :6], ctx=c)
        with pytest.raises(ValueError):
            pipeline.prediction_sequence_dev(fr[:2], _grasp_json_stack(), nsof_lib.dataset_config("grasp", **SMALL), ctx=c)
        # the C entries check before launching: W < 7, max_rects < 1, a missing table, a short table, no pairs
        d = torch.zeros((2,), dtype=torch.float64, device=torch_dev)
        rc = c._lib.nsof_ssim_u8_batch_dev(c.ptr, 2, fr.data_ptr(), 6 * 3, 32 * 40 * 3, 3, fr.data_ptr(), 6 * 3,
                                           32 * 40 * 3, 3, 6, 32, 255.0, d.data_ptr())
        assert rc == _lib.NSOF_ESHAPE
        counts = torch.zeros((4,), dtype=torch.int32, device=torch_dev)
        rects = torch.zeros((4, 2, 4), dtype=torch.int32, device=torch_dev)
        out = torch.empty((3, 32, 40, 3), dtype=torch.uint8, device=torch_dev)
        torch.cuda.synchronize()

        def warp(n_pairs, cnt, rct, n_maps, max_rects):
            return c._lib.nsof_predict_sequence_u8_dev(c.ptr, n_pairs, fr.data_ptr(), 40 * 3, 32 * 40 * 3, 40, 32,
                                                       fl.data_ptr(), -1, cnt, rct, n_maps, max_rects, 0, -1, 1,
                                                       out.data_ptr())
        assert warp(3, counts.data_ptr(), rects.data_ptr(), 4, 0) == _lib.NSOF_EINVAL
        assert warp(3, counts.data_ptr(), None, 4, 2) == _lib.NSOF_EINVAL
        assert warp(3, counts.data_ptr(), rects.data_ptr(), 2, 2) == _lib.NSOF_ESHAPE
        with pytest.raises(NsofError):
            c.check(warp(0, None, None, 0, 0), "predict_sequence")
        assert c.prof_collect(_lib.K_REMAP)[1] == 0 and c.prof_collect(_lib.K_SSIM)[1] == 0
    finally:
        c.close()
