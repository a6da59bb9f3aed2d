#!/usr/bin/env python3
"""Monte-Carlo device trials of the event-driven accumulator on the stream of scripts/bench_accum_maps.py at 1280x720 (1 M
events over 1 s, 1 ms slices, scheme 1, active_v = -6, silent_v = 0: the dead zone), 10 % spread on kon, koff, Ron, Roff, a
block-current map of 80 x 80 pixel blocks after every 33rd slice (31 maps per trial), T in {1, 16, 64} trials:
  trials  ONE nsof.simulate_trials_dev call (nsof_accum_trials_dev): planes checked and uploaded, the stream scattered and
          resolved once per group, T states replayed, T x 31 block-current maps left in HBM
  loop    what it replaces: T times Accumulator(param_maps=planes[t]), step(snap_every=33), block_current_dev of every
          snapshot into one [T][31][rows][cols] tensor, close -- the existing single-array path
Both start from the same host arrays (events, [T][H][W] float32 planes drawn before the clock starts) and end in a device
synchronise with their maps in HBM; the two stacks are compared bit for bit once per process.

Two ways to call it.
  worker   bench_accum_trials.py --what trials|loop [--tree DIR]      one process, one JSON line.  --tree DIR measures the
           package under DIR (a checkout of another commit with its own libnsof.so), for a parent-against-branch comparison
  session  bench_accum_trials.py --session [--rounds 3] [--out profiles/accum_trials.json]
           starts the two kinds of worker alternately, `rounds` times in fresh processes, and writes the medians over the
           processes with their min-max spread and, per T, whether the trial run's median stays below the loop's minimum.

Timing: the host clock around the whole call(s); one untimed warm-up, then `reps` timed repetitions; a process reports its
median."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_accum_maps import SPREAD_KEYS, stream  # noqa: E402

W, H, EVERY, MEMSIZE = 1280, 720, 33, 80
TRIALS = (1, 16, 64)


def worker(a):
    root = os.path.abspath(a.tree)
    sys.path[:0] = [root, os.path.join(root, "neuromorphic-spatiotemporal-optical-flow_amd")]
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch
    import nsof
    from nsof import accumulator as A  # noqa: N812
    ctx = nsof.Context(0)
    dev = torch.device("cuda", ctx.device)
    ev = stream(np, W, H)
    idx = A.slice_index_array(ev[3], 1000)
    n_sl = len(idx) - 1
    n_snap = (n_sl - 1) // EVERY + 1
    rows, cols = H // MEMSIZE, W // MEMSIZE
    out = {"what": a.what, "tree": root, "lib": nsof._lib.LIB_PATH, "reps": a.reps, "slices": n_sl, "snapshots": n_snap, "trials": {}}

    def trials_run(maps):
        return A.simulate_trials_dev(ev, maps, 1, 1000, -6.0, 0.0, sensor_size=(H, W), snapshot_every=EVERY, memsize=MEMSIZE,
                                     ctx=ctx)["block_current"][0]

    def loop_run(maps):
        n_t = next(iter(maps.values())).shape[0]
        cur = torch.empty((n_t, n_snap, rows, cols), dtype=torch.float64, device=dev)
        for t in range(n_t):
            acc = A.Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx, param_maps={k: v[t] for k, v in maps.items()})
            acc.step(*ev, idx, snap_every=EVERY)
            for s in range(n_snap):
                acc.block_current_dev(MEMSIZE, cur[t, s], snapshot=s)
            ctx.synchronize()
            acc.close()
        return cur

    call = trials_run if a.what == "trials" else loop_run
    for n_t in a.trials:
        maps = A.variability_maps(H, W, {k: 0.1 for k in SPREAD_KEYS}, None, seed=1, trials=n_t)
        got = call(maps)                                  # warm-up: allocations, code objects
        ctx.synchronize()
        ms = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call(maps)
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        other = (loop_run if a.what == "trials" else trials_run)(maps) if n_t <= a.check_up_to else None
        ctx.synchronize()
        out["trials"][str(n_t)] = {"ms": round(statistics.median(ms), 2), "min": round(min(ms), 2), "max": round(max(ms), 2),
                                   "checksum": float(got.sum().item()),
                                   "same_bits_as_the_other_form": None if other is None else bool(torch.equal(got, other))}
    ctx.close()
    print(json.dumps(out))


def session(a):
    me = os.path.abspath(__file__)

    def run(what):
        cmd = [sys.executable, me, "--what", what, "--reps", str(a.reps), "--trials", ",".join(str(t) for t in a.trials),
               "--check-up-to", str(a.check_up_to)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, check=True)
        print(r.stdout.strip().splitlines()[-1], file=sys.stderr, flush=True)   # progress: a session takes minutes
        return json.loads(r.stdout.strip().splitlines()[-1])
    runs = {"trials": [], "loop": []}
    for _ in range(a.rounds):                            # alternating: other work shares the machine
        for what in ("loop", "trials"):
            runs[what].append(run(what))

    def summary(rs, n_t):
        v = [r["trials"][str(n_t)]["ms"] for r in rs]
        return {"ms": statistics.median(v), "min": min(v), "max": max(v), "per_process": v,
                "checksums": sorted({r["trials"][str(n_t)]["checksum"] for r in rs}),
                "same_bits_as_the_other_form": sorted({str(r["trials"][str(n_t)]["same_bits_as_the_other_form"]) for r in rs})}
    out = {"workload": f"1e6 events over 1 s on {W}x{H}, 1 ms slices, scheme 1, active_v=-6, silent_v=0, 10 % spread on "
                       + ", ".join(SPREAD_KEYS) + f", block currents of {MEMSIZE}x{MEMSIZE} blocks after every {EVERY}rd slice; "
                       "trials = one simulate_trials_dev call, loop = T x (Accumulator(param_maps=), step, block_current_dev per snapshot)",
           "method": f"{a.rounds} alternating fresh processes per form; per process one warm-up and the median of {a.reps} timed "
                     "repetitions of the whole call(s), host clock, planes drawn beforehand; figures are the median over the "
                     "processes, min / max their spread", "by_trials": {}}
    for n_t in a.trials:
        tr, lo = summary(runs["trials"], n_t), summary(runs["loop"], n_t)
        out["by_trials"][str(n_t)] = {"trials": tr, "loop": lo, "loop_over_trials": round(lo["ms"] / tr["ms"], 3),
                                      "trials_median_at_most_loop_min": bool(tr["ms"] <= lo["min"]),
                                      "same_checksum": tr["checksums"] == lo["checksums"]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("trials", "loop"), default="trials")
    ap.add_argument("--session", action="store_true")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--trials", default=TRIALS, type=lambda s: tuple(int(v) for v in s.split(",")))
    ap.add_argument("--check-up-to", type=int, default=16, help="compare the two forms' stacks bit for bit up to this many trials")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=900)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (session if args.session else worker)(args)
