#!/usr/bin/env python3
"""The segmentation experiment of optical_flow_seg.py over a whole sequence on the device; prints one JSON line.

    python scripts/bench_segment_sequence.py [--frames 32 --reps 5 --host-frames 6 --out <file>]

A seeded synthetic sequence of the grasp frame size (1920 x 1080, ``workload.synthetic_sequence`` replicated to 3
channels) with seeded ground-truth frames, gated by the grasp slices of tests/golden/gating_stacks.npz (FLAG 2,
parameter set A).
  device:   ``pipeline.segmentation_sequence_dev`` (frames in HBM, results in HBM): wall time per pair after a warm-up
            call, split into the flow stage (gray frames, gating table, ROI and full-frame flows) and the mask +
            accuracy stage of each path (``timings``)
  head:     the mask stages alone on the flows of that call: ``segment.motion_mask_sequence_dev`` (boxes, then whole
            frame) and ``segment.pixel_accuracy_batch_dev`` of each path
  host:     ``pipeline.run_segmentation`` with the GPU backends on the first --host-frames frames (numpy in, rows out)
  bytes:    the byte model per pair of the mask stages: pack 8 B/px of flow inside the boxes (whole frame for the
            Original path), compose 1 B/px written, accuracy 4 B/px read (mask + BGR ground truth); the bit images
            (1/8 B/px per pass) are left out"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=6)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import gating, pipeline, segment
    from nsof import workload as wl
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    h, w = wl.DATASET_FRAMES["grasp"][:2]
    n = a.frames
    with np.load(os.path.join(ROOT, "tests", "golden", "gating_stacks.npz")) as z:
        stack = z["grasp"]
    frames = [np.ascontiguousarray(np.repeat(f[..., None], 3, 2)) for f in wl.synthetic_sequence(2024, n, h, w)]
    rng = np.random.default_rng(7)
    gts = [np.where(rng.random((h, w, 1)) < 0.1, np.uint8(255), np.uint8(0)).repeat(3, 2) for _ in range(n)]
    d_frames = torch.from_numpy(np.stack(frames)).to(dev)
    d_gts = torch.from_numpy(np.stack(gts)).to(dev)
    torch.cuda.synchronize()
    cfg = gating.dataset_config("grasp")

    res = pipeline.segmentation_sequence_dev(d_frames, d_gts, stack, cfg, ctx=ctx)   # warm-up
    tm = {}
    stages = {"flow_s": 0.0, "seg_mem_s": 0.0, "seg_orig_s": 0.0}
    t0 = time.perf_counter()
    for _ in range(a.reps):
        res = pipeline.segmentation_sequence_dev(d_frames, d_gts, stack, cfg, ctx=ctx, timings=tm)
        for k in stages:
            stages[k] += tm[k] / a.reps
    dt_dev = (time.perf_counter() - t0) / a.reps
    n_pairs = n - 2

    def head():
        segment.motion_mask_sequence_dev(res["flow_mem"], res["boxes"], res["mask_mem"], ctx=ctx)
        segment.pixel_accuracy_batch_dev(res["mask_mem"], d_gts[1:n - 1], res["pa_mem"], ctx=ctx)
        segment.motion_mask_sequence_dev(res["flow_orig"], None, res["mask_orig"], ctx=ctx)
        segment.pixel_accuracy_batch_dev(res["mask_orig"], d_gts[1:n - 1], res["pa_orig"], ctx=ctx)

    head()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        head()
    ctx.synchronize()
    dt_head = (time.perf_counter() - t0) / a.reps

    hn = max(3, min(a.host_frames, n))
    t0 = time.perf_counter()
    _, m_mem, m_orig = pipeline.run_segmentation(frames[:hn], gts[:hn], stack, gating.dataset_config("grasp"))
    dt_host = time.perf_counter() - t0
    pm, po = res["pa_mem"].cpu().tolist()[:hn - 2], res["pa_orig"].cpu().tolist()[:hn - 2]
    same = sum(pm) / len(pm) == m_mem and sum(po) / len(po) == m_orig

    roi = float(np.mean([sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in b) / (h * w) for b in res["boxes"]]))
    px = h * w
    model = {"mask_mem": (8 * roi + 1) * px, "mask_orig": 9.0 * px, "accuracy": 4.0 * px}
    out = {"bench": "segment_sequence", "frame_hw": [h, w], "frames": n, "pairs": n_pairs, "reps": a.reps,
           "device_ms_per_pair": round(dt_dev / n_pairs * 1e3, 3), "device_ms_per_run": round(dt_dev * 1e3, 2),
           "stage_ms_per_pair": {k[:-2]: round(v / n_pairs * 1e3, 3) for k, v in stages.items()},
           "head_us_per_pair": round(dt_head / n_pairs * 1e6, 2),
           "host_ms_per_pair": round(dt_host / (hn - 2) * 1e3, 2), "host_pairs": hn - 2,
           "host_means_equal_device": bool(same), "roi_fraction": round(roi, 4),
           "byte_model_per_pair": {k: int(v) for k, v in model.items()} |
           {"total": int(model["mask_mem"] + model["mask_orig"] + 2 * model["accuracy"])},
           "head_bytes_per_s_of_model": round((model["mask_mem"] + model["mask_orig"] + 2 * model["accuracy"]) /
                                              (dt_head / n_pairs), 1),
           "mean_mem": res["mean_mem"], "mean_orig": res["mean_orig"]}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
