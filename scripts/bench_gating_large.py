#!/usr/bin/env python3
"""Device ROI gating of large maps; prints one JSON line and writes it to --out.

    python scripts/bench_gating_large.py [--maps 32 --reps 10 --out profiles/gating_large_bench.json]

  gating:  ``gating.roi_from_surface_dev`` on a batch of --maps seeded maps (ON density --density, near percolation) at
           36x64 (one wavefront per map), 108x192 (3840x2160 at MEMSIZE 20), 216x384 and 540x960 cells, FLAG 1 and FLAG 2,
           4-connectivity; wall time per batch after a warm-up call (synchronised), per map, next to the host C mirror
           ``gating.roi_from_surface`` on the same maps (one map after the other), and the equality of the two tables
  stream:  ``pipeline.events_to_roi_flows`` on ``synth.make_event_stream_4k`` (3840x2160, 1 M events, 1000 slices of
           1 ms, silent 0.5 V) at MEMSIZE 20 (108 x 192 cells), FLAG 1, parameter set A: its ``timings`` after a
           warm-up call -- surface + gating and the ROI flow stage"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--density", type=float, default=0.55)
    ap.add_argument("--stream-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gating_large_bench.json"))
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import gating, pipeline, synth
    from nsof.farneback import PARAMS_A
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    rng = np.random.default_rng(2024)
    rec = {"workload": f"{a.maps} maps per batch, ON density {a.density}, THRES 200, MEMSIZE 20, CONNECT 4", "gating": [],
           "stream": None}
    for rows, cols in ((36, 64), (108, 192), (216, 384), (540, 960)):
        on = rng.random((a.maps, rows, cols)) < a.density
        cur = np.where(on, 1e-5, 1e-9)                # gray 255 vs 68
        d = torch.from_numpy(cur).to(dev)
        torch.cuda.synchronize()
        fh, fw = rows * 20, cols * 20
        for flag in (1, 2):
            cfg = gating.GatingConfig(MEMSIZE=20, THRES=200, FLAG=flag, CONNECT=4)
            t0 = time.perf_counter()
            want = [gating.roi_from_surface(cur[k], (fh, fw), cfg) for k in range(a.maps)]
            dt_host = (time.perf_counter() - t0) / a.maps
            cap = max(1, max(len(v) for v in want))
            out = gating.roi_from_surface_dev(d, a.maps, (rows, cols), (fh, fw), cfg, max_rects=cap, ctx=ctx)   # warm-up
            same = gating.rects_to_host(*out, ctx=ctx) == want
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                gating.roi_from_surface_dev(d, a.maps, (rows, cols), (fh, fw), cfg, max_rects=cap, ctx=ctx)
            ctx.synchronize()
            dt_dev = (time.perf_counter() - t0) / a.reps
            rec["gating"].append({"map": f"{rows}x{cols}", "flag": flag, "components_per_map": float(np.mean([len(v) for v in want])),
                                  "device_ms_per_batch": round(dt_dev * 1e3, 4),
                                  "device_us_per_map": round(dt_dev / a.maps * 1e6, 3),
                                  "host_mirror_us_per_map": round(dt_host * 1e6, 3),
                                  "host_over_device": round(dt_host / (dt_dev / a.maps), 2), "tables_equal": bool(same)})
        del d

    H, W = 2160, 3840  # noqa: N806
    x, y, p, t = synth.make_event_stream_4k()
    cfg = gating.GatingConfig(MEMSIZE=20, EXTEND_HEIGHT_UPPER=20, EXTEND_HEIGHT_LOWER=20, EXTEND_WIDTH_LEFT=20,
                              EXTEND_WIDTH_RIGHT=20, THRES=240, FLAG=1, farneback_params=PARAMS_A)
    kw = dict(slice_us=1000, active_v=-6.0, silent_v=0.5, snapshot_every=33, ctx=ctx, max_rects=256)
    pipeline.events_to_roi_flows(x, y, p, t, (H, W), cfg, **kw)     # warm-up
    acc = {"surface_and_gating_s": 0.0, "flow_s": 0.0}
    for _ in range(a.stream_reps):
        tm = {}
        frames, rects, flows = pipeline.events_to_roi_flows(x, y, p, t, (H, W), cfg, timings=tm, **kw)
        for k in acc:
            acc[k] += tm[k] / a.stream_reps
    del frames, flows
    rec["stream"] = {"sensor": f"{W}x{H}", "events": int(len(t)), "memsize": 20, "map": f"{H // 20}x{W // 20}",
                     "frames": tm["frames"], "roi_calls": tm["roi_calls"], "roi_pixels": tm["roi_pixels"],
                     "rois_per_frame_max": max(len(r) for r in rects),
                     "surface_and_gating_ms": round(acc["surface_and_gating_s"] * 1e3, 3),
                     "flow_ms": round(acc["flow_s"] * 1e3, 3)}
    ctx.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
