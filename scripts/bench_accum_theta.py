#!/usr/bin/env python3
"""Scheme 1's event-count threshold on the stream of scripts/bench_accum.py (BASELINE config 5: 3840x2160, 1 M events/s,
1 ms slices, a surface frame every 33 slices): slices/s at theta = 1, 2, 3, 8 on three routes --
  event_pixel  the event-pixel update over the whole stream (dense=False, Accumulator.run)
  every_pixel  the every-pixel pass, a frame per interval (dense=True, Accumulator.run_frames)
  run_frames   nsof_accum_run_frames as it chooses (theta 1: the tile walk; theta > 1: copy + patch, an interval in several rounds)

Two ways to call it.
  worker   bench_accum_theta.py [--tree DIR] [--thetas 1,2,3,8]      one process, one JSON line.  --tree DIR measures the
           package under DIR (a checkout of another commit with its own libnsof.so; a tree without the threshold takes
           --thetas 1, for which no keyword is passed).
  session  bench_accum_theta.py --parent DIR [--rounds 3] [--out profiles/accum_theta_bench.json]
           starts workers alternately -- parent at theta 1, this tree at every theta -- `rounds` times in fresh processes,
           and writes the medians over the rounds with their min-max spread, this tree's theta = 1 against the parent's, and
           the ratio of every theta to theta = 1.

Timing: the host clock around calls that end in a device synchronise; every (route, theta) is warmed up by one untimed
call, then timed in `reps` windows of at least `--window` seconds of back-to-back calls (the state saturates but the
arithmetic per driven slice is the same); a window's figure is slices / time, a process reports the median window."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("event_pixel", "every_pixel", "run_frames")


def worker(a):
    root = os.path.abspath(a.tree)
    sys.path[:0] = [root, os.path.join(root, "neuromorphic-spatiotemporal-optical-flow_amd")]
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import nsof
    import torch
    from nsof.accumulator import Accumulator, slice_index_array
    W, H, n, every = 3840, 2160, 1_000_000, 33  # noqa: N806
    rng = np.random.default_rng(5)                      # the stream of scripts/bench_accum.py
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    k = int(0.3 * n)
    t = np.sort(rng.integers(0, 1_000_000, n)).astype(np.int64)
    drift = (t[:k] * 600e-6).astype(np.int64)
    x[:k] = (rng.integers(0, 400, k) + drift) % W
    y[:k] = rng.integers(0, 300, k) + H // 3
    p = rng.integers(0, 2, n)
    x, y, p = x.astype(np.int16), y.astype(np.int16), p.astype(np.int8)
    idx = slice_index_array(t, 1000)
    n_sl = len(idx) - 1
    n_fr = n_sl // every
    ctx = nsof.Context(0)
    frames = torch.empty((n_fr, H, W), dtype=torch.uint8, device=torch.device("cuda", 0))
    out = {"tree": root, "lib": nsof._lib.LIB_PATH, "slices": n_sl, "frames": n_fr, "reps": a.reps, "window_s": a.window,
           "routes": {r: {} for r in ROUTES}}

    def timed(call, slices):
        call()                                           # warm-up: allocations, code objects
        ctx.synchronize()
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        inner = max(1, int(a.window / max(time.perf_counter() - t0, 1e-6)) + 1)
        rates = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(inner):
                call()
            ctx.synchronize()
            rates.append(inner * slices / (time.perf_counter() - t0))
        return {"slices_per_s": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1),
                "calls_per_window": inner}

    for theta in a.thetas:
        kw = {} if theta == 1 else dict(theta_events=theta)
        for route in ROUTES:
            acc = Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx, dense={"event_pixel": False, "every_pixel": True,
                                                                           "run_frames": None}[route], **kw)
            acc.set_events(x, y, p, t, idx)
            if route == "event_pixel":
                call, slices = (lambda: acc.run(0, n_sl)), n_sl
            else:
                call, slices = (lambda: acc.run_frames(0, n_fr, every, frames)), n_fr * every
            res = timed(call, slices)
            acc.reset()                                      # one run from the initial state: what the result is compared by
            call()
            ctx.synchronize()
            res["checksum"] = [float(acc.w(0).astype("float64").sum()),
                               0 if route == "event_pixel" else int(frames.to(torch.int64).sum().item())]
            out["routes"][route][str(theta)] = res
            acc.close()
    ctx.close()
    print(json.dumps(out))


def session(a):
    me = os.path.abspath(__file__)

    def run(tree, thetas):
        cmd = [sys.executable, me, "--tree", tree, "--thetas", ",".join(map(str, thetas)), "--reps", str(a.reps),
               "--window", str(a.window)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, check=True)
        return json.loads(r.stdout.strip().splitlines()[-1])
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):                            # alternating: other work shares the machine
        runs["parent"].append(run(a.parent, [1]))
        runs["this"].append(run(HERE, a.thetas))

    def summary(rs, route, theta):
        v = [r["routes"][route][str(theta)]["slices_per_s"] for r in rs]
        return {"slices_per_s": statistics.median(v), "min": min(v), "max": max(v), "per_process": v,
                "checksums": sorted({tuple(r["routes"][route][str(theta)]["checksum"]) for r in rs})}
    out = {"workload": "3840x2160, 1e6 events over 1 s, 1 ms slices, scheme 1, active_v=-6, silent_v=0, a frame every 33 slices",
           "method": f"{a.rounds} alternating fresh processes per tree; per process the median of {a.reps} windows of >= "
                     f"{a.window} s after one warm-up call; figures are the median over the processes, min / max their spread",
           "parent": {}, "this": {}, "theta1_vs_parent": {}, "ratio_to_theta1": {}}
    for route in ROUTES:
        out["parent"][route] = {"1": summary(runs["parent"], route, 1)}
        out["this"][route] = {str(th): summary(runs["this"], route, th) for th in a.thetas}
        par, one = out["parent"][route]["1"], out["this"][route]["1"]
        spread = max(par["max"] - par["min"], one["max"] - one["min"])
        out["theta1_vs_parent"][route] = {
            "ratio": round(one["slices_per_s"] / par["slices_per_s"], 4),
            "difference": round(one["slices_per_s"] - par["slices_per_s"], 1), "run_to_run_spread": round(spread, 1),
            "inside_spread": bool(par["slices_per_s"] - one["slices_per_s"] <= spread),
            "same_checksum": one["checksums"] == par["checksums"]}
        out["ratio_to_theta1"][route] = {str(th): round(out["this"][route][str(th)]["slices_per_s"] / one["slices_per_s"], 4)
                                         for th in a.thetas}
    line = json.dumps(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(out, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent", default=None, help="session mode: a checkout of the parent commit with its own libnsof.so")
    ap.add_argument("--thetas", default="1,2,3,8", type=lambda s: [int(v) for v in s.split(",")])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=280)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (session if args.parent else worker)(args)
