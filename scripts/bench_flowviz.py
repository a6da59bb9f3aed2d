#!/usr/bin/env python3
"""Middlebury colour coding of flow fields on the device (``flowviz.flow_to_image_dev``); prints one JSON line.

    python scripts/bench_flowviz.py [--frames 32 --batch 32 --reps 100 --host-flows 2 --kernel-stats <kernel_stats.csv>]
                                    [--out profiles/flowviz_bench.json]

Flows: the Farneback flows of the ``bench_predict_sequence.py`` workload (a seeded synthetic 1920 x 1080 sequence gated
by the grasp slices of tests/golden/gating_stacks.npz, FLAG 2, parameter set A): the full-frame flows, then the gated
ones, the first --batch of them as one [batch][1080][1920][2] tensor.
  device:   us per flow of one batched call, each flow normalised by its own max (``max``) and with ``max_flow`` given
            (``given``), host clock around --reps calls that ends in a synchronise, after a warm-up call of each
  bytes:    the byte model per pixel: the max pass reads 8 B, the colour pass reads 8 B and writes 3 B (19 B/px; 11 B/px
            with max_flow), and its share of 8 TB/s at the measured time
  host:     ``nsof.flow_to_image`` (the NumPy mirror) on the first --host-flows flows, ms per flow, and the pixels where
            it differs from the device (its float32 arctan2 is not correctly rounded)
  viz:      extra device time per pair of ``prediction_sequence_dev(with_viz=True)`` over ``with_viz=False`` (the two
            alternated, --seq-reps runs each)
With --kernel-stats (the kernel_stats.csv of a separate ``rocprofv3 --kernel-trace --stats`` run of this script with
--trace) the average launch time of each kernel, per flow and its share of 8 TB/s follow.  --trace runs the two batched
calls --reps times and nothing else."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]
HBM_PEAK = 8e12
BYTES_MAX, BYTES_COLOR = 8.0, 11.0     # per pixel


def kernel_times(path):
    """kernel -> (calls, average ns) from a rocprofv3 kernel_stats.csv (the colour pass split by its GIVEN argument)."""
    keys = {"k_flowviz_max": "max_pass", "k_flowviz_color<true, false, false>": "color_pass",
            "k_flowviz_color<true, false, true>": "color_pass_given"}
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            for frag, key in keys.items():
                if frag in row["Name"]:
                    out[key] = (int(row["Calls"]), float(row["AverageNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--seq-reps", type=int, default=5)
    ap.add_argument("--host-flows", type=int, default=2)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import flowviz, gating, pipeline
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
    res = pipeline.prediction_sequence_dev(d_frames, stack, cfg, ctx=ctx, with_viz=True)   # warm-up, and the flows
    flows = torch.cat([res["flow_orig"], res["flow_mem"]])[:a.batch].contiguous()
    b = int(flows.shape[0])
    out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def run(max_flow):
        flowviz.flow_to_image_dev(flows, out, max_flow=max_flow, ctx=ctx)

    given = float(torch.linalg.vector_norm(flows, dim=-1).max().item())
    if a.trace:
        for _ in range(a.reps):
            run(None)
            run(given)
        ctx.synchronize()
        print(json.dumps({"bench": "flowviz", "trace_reps": a.reps, "batch": b}))
        return

    timing = {}
    for mode, mf in (("max", None), ("given", given)):
        run(mf)
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            run(mf)
        ctx.synchronize()
        timing[mode] = (time.perf_counter() - t0) / a.reps / b

    # the per-flow max images of the first flows against the host mirror
    run(None)
    ctx.synchronize()
    dev_img = out[:a.host_flows].cpu().numpy()
    host_flows = flows[:a.host_flows].cpu().numpy()
    t0 = time.perf_counter()
    host_img = [nsof.flow_to_image(f) for f in host_flows]
    dt_host = (time.perf_counter() - t0) / max(len(host_img), 1)
    diff = np.stack([np.abs(d.astype(np.int16) - hi).max(-1) for d, hi in zip(dev_img, host_img)])

    # extra device time of the two viz calls inside the sequence experiment
    seq = {False: 0.0, True: 0.0}
    for _ in range(a.seq_reps):
        for with_viz in (False, True):
            t0 = time.perf_counter()
            pipeline.prediction_sequence_dev(d_frames, stack, cfg, ctx=ctx, with_viz=with_viz)
            seq[with_viz] += time.perf_counter() - t0
    n_pairs = n - 2
    px = h * w
    model = {"max": BYTES_MAX + BYTES_COLOR, "given": BYTES_COLOR}
    line = {"bench": "flowviz", "frame_hw": [h, w], "batch": b, "reps": a.reps,
            "us_per_flow": {k: round(v * 1e6, 2) for k, v in timing.items()},
            "byte_model_per_px": model,
            "hbm_share": {k: round(model[k] * px / timing[k] / HBM_PEAK, 4) for k in timing},
            "host_ms_per_flow": round(dt_host * 1e3, 1), "host_flows": len(host_img),
            "host_over_device": round(dt_host / timing["max"], 0),
            "mirror_diff_px": int(np.count_nonzero(diff)), "mirror_diff_max_level": int(diff.max()),
            "sequence_pairs": n_pairs,
            "sequence_ms_per_run": {"with_viz": round(seq[True] / a.seq_reps * 1e3, 2),
                                    "without": round(seq[False] / a.seq_reps * 1e3, 2)},
            "viz_extra_us_per_pair": round((seq[True] - seq[False]) / a.seq_reps / n_pairs * 1e6, 2)}
    if a.kernel_stats:
        kt = kernel_times(a.kernel_stats)
        kb = {"max_pass": BYTES_MAX, "color_pass": BYTES_COLOR, "color_pass_given": BYTES_COLOR}
        line["kernels"] = {k: {"calls": c, "avg_us": round(ns / 1e3, 2), "us_per_flow": round(ns / 1e3 / b, 3),
                               "hbm_share": round(kb[k] * px * b / (ns * 1e-9) / HBM_PEAK, 4)}
                           for k, (c, ns) in kt.items()}
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
