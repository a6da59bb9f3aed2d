#!/usr/bin/env python3
"""The prediction experiment of optical_flow_prediction.py over a whole sequence on the device; prints one JSON line.

    python scripts/bench_predict_sequence.py [--frames 32 --reps 5 --host-frames 6 --kernel-stats <kernel_stats.csv>]

A seeded synthetic sequence of the grasp frame size (1920 x 1080, ``workload.synthetic_sequence`` replicated to 3
channels) gated by the grasp slices of tests/golden/gating_stacks.npz (FLAG 2, parameter set A).
  device:   ``pipeline.prediction_sequence_dev`` (frames in HBM, results in HBM), pairs/s after a warm-up call;
            ``head``: the prediction head alone (two batched warps + two batched SSIMs on the flows of that call)
  host:     ``pipeline.run_prediction`` with the GPU backends on the first --host-frames frames (numpy in, CSV rows out)
  bytes:    the byte model per pair: mem warp 6 B/px (frame in, prediction out) + 8 B/px of flow inside the warped box,
            original warp 14 B/px, each SSIM 6 B/px (the interleaved lines of both frames)
With --kernel-stats (the kernel_stats.csv of a separate ``rocprofv3 --kernel-trace --stats`` run of this script with
--trace) the average launch time of each kernel and its share of 8 TB/s follow from that model.  --trace runs the device
experiment --reps times and nothing else."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]
HBM_PEAK = 8e12


def kernel_times(path):
    """name fragment -> (calls, average ns) from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            for key in ("k_predict_seq_u8<true>", "k_predict_seq_u8<false>", "k_ssim_partial", "k_ssim_final"):
                if key in row["Name"]:
                    out[key] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=6)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import gating, pipeline, predict
    from nsof import workload as wl
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    h, w = wl.DATASET_FRAMES["grasp"][:2]
    n = a.frames
    with np.load(os.path.join(ROOT, "tests", "golden", "gating_stacks.npz")) as z:
        stack = z["grasp"]
    frames = [np.ascontiguousarray(np.repeat(f[..., None], 3, 2)) for f in wl.synthetic_sequence(2024, n, h, w)]
    d_frames = torch.from_numpy(np.stack(frames)).to(dev)
    torch.cuda.synchronize()
    cfg = gating.dataset_config("grasp")

    res = pipeline.prediction_sequence_dev(d_frames, stack, cfg, ctx=ctx)   # warm-up
    if a.trace:
        for _ in range(a.reps):
            pipeline.prediction_sequence_dev(d_frames, stack, cfg, ctx=ctx)
        print(json.dumps({"bench": "predict_sequence", "trace_runs": a.reps + 1, "frames": n}))
        return
    t0 = time.perf_counter()
    for _ in range(a.reps):
        res = pipeline.prediction_sequence_dev(d_frames, stack, cfg, ctx=ctx)
    dt_dev = (time.perf_counter() - t0) / a.reps
    n_pairs = n - 2

    # the head alone: both warps and both SSIMs of every pair from the flows already in HBM
    counts, rtab = gating.roi_from_surface_dev(
        torch.from_numpy(np.ascontiguousarray(np.moveaxis(stack[:, :, :n - 1], 2, 0))).to(dev), n - 1, stack.shape[:2],
        (h, w), cfg, ctx=ctx)
    ctx.synchronize()

    def head():
        predict.predict_sequence_dev(d_frames, res["flow_mem"], res["pred_mem"], counts=counts, rects=rtab, ctx=ctx)
        predict.ssim_batch_dev(res["pred_mem"], d_frames[2:], out=res["ssim_mem"], ctx=ctx)
        predict.predict_sequence_dev(d_frames, res["flow_orig"], res["pred_orig"], border_mode=predict.BORDER_CONSTANT,
                                     ctx=ctx)
        predict.ssim_batch_dev(res["pred_orig"], d_frames[2:], out=res["ssim_orig"], ctx=ctx)

    head()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.reps):
        head()
    ctx.synchronize()
    dt_head = (time.perf_counter() - t0) / a.reps

    hn = max(3, min(a.host_frames, n))
    t0 = time.perf_counter()
    _, s_mem, s_orig, _, _ = pipeline.run_prediction(frames[:hn], stack, gating.dataset_config("grasp"))
    dt_host = time.perf_counter() - t0
    same = bool(np.array_equal(res["ssim_mem"].cpu().numpy()[:hn - 2], np.array(s_mem)) and
                np.array_equal(res["ssim_orig"].cpu().numpy()[:hn - 2], np.array(s_orig)))

    roi = float(np.mean([sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in b) / (h * w) for b in res["boxes"]]))
    px = h * w
    model = {"k_predict_seq_u8<true>": (6 + 8 * roi) * px, "k_predict_seq_u8<false>": 14.0 * px,
             "k_ssim_partial": 6.0 * px}
    out = {"bench": "predict_sequence", "frame_hw": [h, w], "frames": n, "pairs": n_pairs, "reps": a.reps,
           "device_pairs_per_s": round(n_pairs / dt_dev, 1), "device_ms_per_run": round(dt_dev * 1e3, 2),
           "head_us_per_pair": round(dt_head / n_pairs * 1e6, 2),
           "host_pairs_per_s": round((hn - 2) / dt_host, 2), "host_pairs": hn - 2, "host_equals_device_ssim": same,
           "roi_fraction": round(roi, 4),
           "byte_model_per_pair": {k: int(v) for k, v in model.items()} | {"total": int(model["k_predict_seq_u8<true>"] +
                                                                                  model["k_predict_seq_u8<false>"] +
                                                                                  2 * model["k_ssim_partial"])},
           "ssim_mem_mean": float(res["ssim_mem"].mean().item()), "ssim_orig_mean": float(res["ssim_orig"].mean().item())}
    if a.kernel_stats:
        kt = kernel_times(a.kernel_stats)
        out["kernels"] = {k: {"calls": c, "avg_us": round(ns / 1e3, 2), "us_per_pair": round(ns / 1e3 / n_pairs, 3),
                              **({"hbm_share": round(model[k] * n_pairs / (ns * 1e-9) / HBM_PEAK, 4)} if k in model else {})}
                          for k, (c, ns) in kt.items()}
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
