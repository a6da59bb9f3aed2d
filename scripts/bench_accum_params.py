#!/usr/bin/env python3
"""Accumulator update forms on the BASELINE config 5 stream (3840x2160, 1 M events/s, 1 ms slices, a surface frame every 33
slices), slices/s of each: the tile walk and copy + patch (nsof_accum_run_frames), the every-pixel pass per interval, the
event-pixel update, scheme 2 split and magnitude.  One JSON line.

The A/B of the run-time device parameters: `--tree DIR` measures the package under DIR (a checkout of another commit with
its own libnsof.so) through the same calls, so a parent and a candidate are run alternately by the caller
(profiles/accum_params_bench.json).  `--set alpha|wide` runs a non-default device of tests/accum_params_ref.py instead
(trees that take `params=` only)."""
import argparse
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--set", default=None, choices=("alpha", "wide"))
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
ROOT = os.path.abspath(a.tree)
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]
os.environ.setdefault("NSOF_SKIP_BUILD", "1")
import nsof  # noqa: E402
import torch  # noqa: E402
from nsof import synth  # noqa: E402
from nsof.accumulator import Accumulator, slice_index_array  # noqa: E402

model = {}
if a.set:
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import accum_params_ref as R  # noqa: E402,N812
    cfg = R.SETS[a.set]
    model = dict(params=cfg["params"], dt=cfg["dt"], refractory_us=cfg["refractory_us"])

H, W, every = 2160, 3840, 33
x, y, p, t = synth.make_event_stream_4k()
idx = slice_index_array(t, 1000)
n_sl = len(idx) - 1
n_fr = n_sl // every
ctx = nsof.Context(0)
dev = torch.device("cuda", 0)
out = {"tree": os.path.basename(ROOT), "lib": nsof._lib.LIB_PATH, "set": a.set or "default", "slices": n_sl, "frames": n_fr,
       "reps": a.reps}


def timed(acc, call, slices):
    ts = []
    for _ in range(a.reps + 1):      # the first repetition warms up (allocations) and is dropped
        acc.reset()
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        ts.append(time.perf_counter() - t0)
    ts = ts[1:]
    return {"slices_per_s": round(slices / statistics.median(ts), 1), "best_slices_per_s": round(slices / min(ts), 1),
            "median_ms": round(statistics.median(ts) * 1e3, 3)}


frames = torch.empty((n_fr, H, W), dtype=torch.uint8, device=dev)
for name, kw in (("tile_walk", {}), ("copy_patch", dict(frames_path="copy_patch")), ("every_pixel_pass", dict(dense=True))):
    acc = Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx, **kw, **model)
    acc.set_events(x, y, p, t, idx)
    out[name] = timed(acc, lambda: acc.run_frames(0, n_fr, every, frames), n_fr * every)
    out[name]["checksum"] = int(frames.to(torch.int64).sum().item())
    acc.close()
del frames
for name, version, pol, kw in (("event_pixel_update", 1, "split", dict(dense=False)), ("scheme2_split", 2, "split", {}),
                               ("scheme2_magnitude", 2, "magnitude", {})):
    acc = Accumulator(H, W, version, pol, -6.0, 0.0, ctx=ctx, **kw, **model)
    acc.set_events(x, y, p, t, idx)
    out[name] = timed(acc, lambda: acc.run(0, n_sl), n_sl)
    out[name]["checksum"] = float(acc.w(0).astype("float64").sum())
    acc.close()
ctx.close()
print(json.dumps(out))
