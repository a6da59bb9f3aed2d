#!/usr/bin/env python3
"""What cycle-to-cycle write noise costs the event-driven trial run: the T = 64 run of scripts/bench_accum_trials.py (the
1280x720 stream of scripts/bench_accum_maps.py, 1 M events over 1 s, 1 ms slices, scheme 1, active_v = -6, silent_v = 0, 10 %
spread on kon, koff, Ron, Roff, block currents of 80 x 80 blocks after every 33rd slice) in three forms, plus two:
  parent  nsof.simulate_trials_dev of the PARENT commit's tree (--parent DIR: a checkout with its own libnsof.so)
  quiet   this tree, no noise (the NOISE = false kernels: the parent's)
  noisy   this tree, c2c = dict(sigma=0.05, seed=1): one Philox4x32-10 draw per (trial, driven pixel, driven slice)
All start from the same host arrays (events, [T][H][W] float32 planes drawn before the clock starts) and end in a device
synchronise with the [T][31][9][16] stack in HBM.  Those calls spend most of their time on the host (the domain pass over and
the upload of 4 x 64 planes), so the pair is measured once more without any plane -- identical devices, trials = 64, where
the call is the staged stream and the kernels:
  quiet_same, noisy_same   this tree, param_maps = None, trials = 64, without and with the noise

Two ways to call it.
  worker   bench_accum_c2c.py --what parent|quiet|noisy|quiet_same|noisy_same [--tree DIR]      one process, one JSON line
  session  bench_accum_c2c.py --parent DIR [--rounds 3] [--out profiles/accum_c2c.json]
           starts the five kinds of worker alternately, `rounds` times in fresh processes, and writes the medians over the
           processes with their min-max spread, whether the quiet median lies inside the parent's min-max widened once by
           that spread, and the ratios noisy / quiet and noisy_same / quiet_same.

Timing: the host clock around the whole call; one untimed warm-up, then `reps` timed repetitions; a process reports its
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

W, H, EVERY, MEMSIZE, TRIALS = 1280, 720, 33, 80, 64
NOISE = dict(sigma=0.05, seed=1)
FORMS = ("parent", "quiet", "noisy", "quiet_same", "noisy_same")


def worker(a):
    root = os.path.abspath(a.tree)
    sys.path[:0] = [root, os.path.join(root, "neuromorphic-spatiotemporal-optical-flow_amd")]
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import nsof
    from nsof import accumulator as A  # noqa: N812
    ctx = nsof.Context(0)
    ev = stream(np, W, H)
    same = a.what.endswith("_same")
    maps = None if same else A.variability_maps(H, W, {k: 0.1 for k in SPREAD_KEYS}, None, seed=1, trials=a.trials)
    kw = dict(c2c=NOISE) if a.what.startswith("noisy") else {}
    if same:
        kw["trials"] = a.trials

    def call():
        return A.simulate_trials_dev(ev, maps, 1, 1000, -6.0, 0.0, sensor_size=(H, W), snapshot_every=EVERY, memsize=MEMSIZE, ctx=ctx,
                                     **kw)["block_current"][0]
    got = call()                                          # warm-up: allocations, code objects
    ctx.synchronize()
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        call()
        ctx.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    out = {"what": a.what, "tree": root, "lib": nsof._lib.LIB_PATH, "reps": a.reps, "trials": a.trials, "ms": round(statistics.median(ms), 2),
           "min": round(min(ms), 2), "max": round(max(ms), 2), "checksum": float(got.sum().item())}
    ctx.close()
    print(json.dumps(out))


def session(a):
    me = os.path.abspath(__file__)

    def run(what):
        cmd = [sys.executable, me, "--what", what, "--reps", str(a.reps), "--trials", str(a.trials), "--tree",
               a.parent if what == "parent" else HERE]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, check=True)
        print(r.stdout.strip().splitlines()[-1], file=sys.stderr, flush=True)   # progress: a session takes minutes
        return json.loads(r.stdout.strip().splitlines()[-1])
    runs = {f: [] for f in FORMS}
    for _ in range(a.rounds):                            # alternating: other work shares the machine
        for what in FORMS:
            runs[what].append(run(what))

    def summary(rs):
        v = [r["ms"] for r in rs]
        return {"ms": statistics.median(v), "min": min(v), "max": max(v), "per_process": v, "checksums": sorted({r["checksum"] for r in rs})}
    s = {f: summary(runs[f]) for f in FORMS}
    spread = s["parent"]["max"] - s["parent"]["min"]
    out = {"workload": f"1e6 events over 1 s on {W}x{H}, 1 ms slices, scheme 1, active_v=-6, silent_v=0, T = {a.trials} trials with 10 % "
                       "spread on " + ", ".join(SPREAD_KEYS) + f", block currents of {MEMSIZE}x{MEMSIZE} blocks after every {EVERY}rd slice; "
                       f"one simulate_trials_dev call: the parent commit's, this tree's without noise, this tree's with c2c = {NOISE}; "
                       f"quiet_same / noisy_same: this tree without any plane (identical devices, trials = {a.trials}), without and with it",
           "method": f"{a.rounds} alternating fresh processes per form; per process one warm-up and the median of {a.reps} timed "
                     "repetitions of the whole call, host clock, planes drawn beforehand; figures are the median over the processes, "
                     "min / max their spread",
           **s,
           "quiet_vs_parent": {"accepted_from": round(s["parent"]["min"] - spread, 2), "accepted_to": round(s["parent"]["max"] + spread, 2),
                               "inside": bool(s["parent"]["min"] - spread <= s["quiet"]["ms"] <= s["parent"]["max"] + spread),
                               "not_slower": bool(s["quiet"]["ms"] <= s["parent"]["max"] + spread),
                               "ratio_to_parent_median": round(s["quiet"]["ms"] / s["parent"]["ms"], 4),
                               "same_checksum": s["quiet"]["checksums"] == s["parent"]["checksums"]},
           "noisy_over_quiet": round(s["noisy"]["ms"] / s["quiet"]["ms"], 4),
           "noisy_differs_from_quiet": s["noisy"]["checksums"] != s["quiet"]["checksums"],
           "noisy_same_over_quiet_same": round(s["noisy_same"]["ms"] / s["quiet_same"]["ms"], 4),
           "noisy_same_differs_from_quiet_same": s["noisy_same"]["checksums"] != s["quiet_same"]["checksums"]}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=FORMS, default="quiet")
    ap.add_argument("--parent", default=None, help="session mode: a checkout of the parent commit with its own libnsof.so")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--trials", type=int, default=TRIALS)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=900)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (session if args.parent else worker)(args)
