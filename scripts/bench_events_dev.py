#!/usr/bin/env python3
"""What it costs to bring a generated event stream to the host and back; prints one JSON line.

    python scripts/bench_events_dev.py [--frames 34 --reps 9 --out profiles/events_dev_staging.json]

A 1280 x 720 video of --frames frames of drifting texture, 5000 us apart, through generator -> accumulator frames -> flow
(``nsof.pipeline.video_to_flow_sequence``'s stages: threshold 10 grey levels, slices of 1000 us, a surface frame every 5
slices).  Two paths over the same stream, alternating within every round, the one that goes first changing from round to
round; a warm-up of both first, then medians with min-max over --reps rounds, host clock around work that ends in a
synchronise:

  device   the stream stays in HBM: ``slice_index_array`` and ``Accumulator.set_events`` on the generator's tensors
           (``nsof_accum_slice_bounds_dev``, ``nsof_accum_set_events_dev``)
  host     the parent commit's path: ``ev[k].cpu().numpy()`` of the four tensors, then the host entries
           (``nsof_accum_slice_bounds``, ``nsof_accum_set_events``)

  staging      bounds + check + tables + copy, nothing else: from the tensors in HBM to a staged accumulator
  end_to_end   generator, staging, ``run_frames`` and ``farneback_sequence``: from the frames in HBM to the flows
  pcie_bytes   what crosses PCIe in the staging of each path, computed from the shapes (scheme 1: no slice times)

The run asserts that both paths give the same bounds, surface frames and flows.  Reads nothing outside the repository."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]
H, W = 720, 1280
FRAME_US, THRESHOLD, SLICE_US, EVERY = 5000, 10.0, 1000, 5
STREAM_REC = 32   # bytes of the check's record


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=34)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import pipeline, synth
    from nsof.accumulator import slice_index_array
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    frames = torch.from_numpy(synth.make_sequence(7, a.frames, H, W, pad=192)).to(dev)
    gen = dict(frame_us=FRAME_US, threshold=THRESHOLD, p_off=0, ctx=ctx)
    acc_args = dict(slice_us=SLICE_US, snapshot_every=EVERY, ctx=ctx)
    ev = nsof.events_from_frames_dev(frames, **gen)
    ctx.synchronize()
    xs = tuple(ev[k] for k in "xypt")
    n_events = int(xs[0].shape[0])

    def download(stream):
        return tuple(v.cpu().numpy() for v in stream)

    def staging(path):
        """-> (ms, bounds): from the tensors in HBM to a staged accumulator."""
        acc = nsof.Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        stream = xs if path == "device" else download(xs)
        idx = slice_index_array(stream[3], SLICE_US, ctx)
        acc.set_events(*stream, idx)
        ctx.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        acc.close()
        return ms, idx

    def end_to_end(path):
        """-> (ms, surface frames, flows): from the frames in HBM to the flows."""
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if path == "device":
            surfaces, flows, _ = pipeline.video_to_flow_sequence(frames, frame_us=FRAME_US, threshold=THRESHOLD, p_off=0, **acc_args)
        else:
            e = nsof.events_from_frames_dev(frames, **gen)
            ctx.synchronize()
            surfaces, flows = pipeline.events_to_flow_sequence(*download(tuple(e[k] for k in "xypt")), (H, W), **acc_args)
        ctx.synchronize()
        return (time.perf_counter() - t0) * 1e3, surfaces, flows

    first = {}
    for path in ("host", "device"):   # warm-up of every shape both paths use; what they give is compared
        first[path] = (staging(path)[1], *end_to_end(path)[1:])
    assert np.array_equal(first["host"][0], first["device"][0]), "the bounds differ"
    assert torch.equal(first["host"][1], first["device"][1]) and torch.equal(first["host"][2], first["device"][2]), "frames or flows differ"
    idx = first["host"][0]
    n_bounds, n_staged = len(idx), int(idx[-1] - idx[0])
    ms = {(what, path): [] for what in ("staging", "end_to_end") for path in ("host", "device")}
    for r in range(a.reps):
        for what, fn in (("staging", staging), ("end_to_end", end_to_end)):
            for path in (("host", "device"), ("device", "host"))[r % 2]:
                ms[what, path].append(fn(path)[0])
    line = {"bench": "events_dev_staging", "frame_hw": [H, W], "frames": a.frames, "frame_us": FRAME_US, "threshold_grey": THRESHOLD,
            "slice_us": SLICE_US, "snapshot_every": EVERY, "reps": a.reps, "events": n_events, "staged_events": n_staged,
            "slices": n_bounds - 1, "surface_frames": int(first["host"][1].shape[0]), "same_bounds_frames_and_flows": True}
    for what in ("staging", "end_to_end"):
        line[what] = {path: spread(ms[what, path]) for path in ("host", "device")}
        line[what]["host_over_device"] = round(line[what]["host"]["median_ms"] / line[what]["device"]["median_ms"], 3)
    line["pcie_bytes"] = {
        # x, y, p, t down (2 + 2 + 1 + 8 B per event); x, y, p of the staged events and the bounds up
        "host": {"down": 13 * n_events, "up": 5 * n_staged + 8 * n_bounds},
        # the two bounds calls' records and the table down; the bounds up and the check's record down
        "device": {"down": 2 * STREAM_REC + 8 * n_bounds + STREAM_REC, "up": 8 * n_bounds}}
    line["not_measured"] = ["scheme 2 (16 B per slice more come down)", "other frame sizes and event rates", "kernel times (no profiler run)",
                            "a caller-owned stream"]
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
