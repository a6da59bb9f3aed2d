#!/usr/bin/env python3
"""Cycle-to-cycle write noise in the frame-driven gating array (nsof_accum_frames_f64_c2c_dev): what the NOISE arms of
k_frames_run cost, and that the noiseless entries cost what they did.  The grasp grid, 24 columns x 13 rows, 100 compressed
frames, n_sub_steps 1000 -- a 99 000-step dependent chain per thread, one Philox draw per 1000 steps.  Measured:
  uniform  the noiseless uniform entry (simulate_frames_dev without maps; the fitted device and one with koff = 50) and
  mapped   the noiseless T = 256 mapped run (10 % spread on kon, koff, Ron, Roff, float64 planes), both on the parent commit
           and on this tree: same checksums, the ratio to the parent's median, inside the parent's own min-max spread or not;
  noise    on this tree, sigma = 0.05 (both directions) against no noise at T = 16, 256 and 1024, with the planes of
           `mapped` and without planes (trials=T: identical devices).

Two ways to call it.
  worker   bench_frames_c2c.py [--tree DIR] [--configs uniform,mapped,noise]     one process, one JSON line.  --tree DIR
           measures the package under DIR (a checkout of another commit with its own libnsof.so; a tree without the noise
           entry takes --configs uniform,mapped).
  session  bench_frames_c2c.py --parent DIR [--rounds 3] [--out profiles/frames_c2c.json]
           starts workers alternately (the order swapped every round) -- the parent at uniform,mapped, this tree at all three
           -- `rounds` times in fresh processes and writes the medians over the processes with their min-max spread.

Timing: the host clock around calls that end in a device synchronise; every figure is warmed up by one untimed call, then
timed `reps` times; a process reports the median."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = (13, 24)
N_FRAMES, N_SUB = 100, 1000
MAPPED_T = 256
NOISE_TRIALS = (16, 256, 1024)
SPREAD_KEYS = ("kon", "koff", "Ron", "Roff")
SIGMA = 0.05


def worker(a):
    root = os.path.abspath(a.tree)
    sys.path[:0] = [root, os.path.join(root, "neuromorphic-spatiotemporal-optical-flow_amd")]
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch
    import nsof
    from nsof import accumulator as A  # noqa: N812
    ctx = nsof.Context(0)
    dev = torch.device("cuda", 0)
    frames = torch.from_numpy(np.random.default_rng(7).random((N_FRAMES,) + GRID)).to(dev)   # every pair drives every cell
    torch.cuda.synchronize(dev)
    other = dict(A.PARAMS, koff=50.0)
    spread = {k: 0.1 for k in SPREAD_KEYS}
    out = {"tree": root, "lib": nsof._lib.LIB_PATH, "reps": a.reps}

    def measured(reps=None, **kw):
        """One configuration of simulate_frames_dev: warmed up once, timed `reps` times, the checksum of its currents."""
        call = lambda: A.simulate_frames_dev(frames, n_sub_steps=N_SUB, ctx=ctx, **kw)  # noqa: E731
        call()                                           # warm-up: allocations, code objects
        ctx.synchronize()
        ts = []
        for _ in range(reps or a.reps):
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        cur = call()[2]
        ctx.synchronize()
        return {"ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3),
                "checksum": float(cur.sum().item())}

    def planes(T):  # noqa: N803
        return A.variability_maps(GRID[0], GRID[1], spread, other, seed=1, trials=T, dtype=np.float64)

    if "uniform" in a.configs:
        out["uniform"] = {name: measured(a.uniform_reps, params=params) for name, params in (("fitted", None), ("koff50", other))}
    if "mapped" in a.configs:
        out["mapped"] = measured(params=other, param_maps=planes(MAPPED_T))
    if "noise" in a.configs:
        out["noise"] = {}
        c2c = dict(sigma=SIGMA, seed=1)
        for T in NOISE_TRIALS:  # noqa: N806
            maps = planes(T)
            out["noise"][str(T)] = {
                "planes": {"off": measured(params=other, param_maps=maps), "on": measured(params=other, param_maps=maps, c2c=c2c)},
                "no_planes": {"off": measured(params=other, trials=T), "on": measured(params=other, trials=T, c2c=c2c)}}
    ctx.close()
    print(json.dumps(out))


def session(a):
    me = os.path.abspath(__file__)

    def run(tree, configs):
        cmd = [sys.executable, me, "--tree", tree, "--configs", ",".join(configs), "--reps", str(a.reps), "--uniform-reps",
               str(a.uniform_reps)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, check=True)
        print(f"worker done: {tree} {configs}", file=sys.stderr, flush=True)
        return json.loads(r.stdout.strip().splitlines()[-1])
    runs = {"parent": [], "this": []}
    for i in range(a.rounds):                            # alternating, the order swapped every round: other work shares the machine
        for which in (("parent", "this"), ("this", "parent"))[i % 2]:
            runs[which].append(run(a.parent, ["uniform", "mapped"]) if which == "parent" else run(HERE, ["uniform", "mapped", "noise"]))

    def summary(values):
        return {"ms": statistics.median(values), "min_ms": min(values), "max_ms": max(values), "per_process": values}

    def against_parent(pick):
        par, one = summary([pick(r)["ms"] for r in runs["parent"]]), summary([pick(r)["ms"] for r in runs["this"]])
        return {"parent": par, "this": one, "ratio_to_parent_median": round(one["ms"] / par["ms"], 4),
                "inside_parent_min_max": bool(par["min_ms"] <= one["ms"] <= par["max_ms"]),
                "not_slower_than_parent_max": bool(one["ms"] <= par["max_ms"]),
                "same_checksum": sorted({pick(r)["checksum"] for r in runs["parent"]}) == sorted({pick(r)["checksum"] for r in runs["this"]})}
    out = {"workload": f"grid {GRID[1]}x{GRID[0]} (grasp), {N_FRAMES} frames, n_sub_steps {N_SUB}, dt 5e-4, th1 0.7, th2 1.5; uniform random "
                       "frames (every pair drives every cell); mapped / noise: params with koff=50, planes = 10 % spread on "
                       + ", ".join(SPREAD_KEYS) + f"; noise: sigma {SIGMA} on both branches, seed 1",
           "method": f"{a.rounds} alternating fresh processes per tree; per process the median of {a.reps} timed calls "
                     f"({a.uniform_reps} for the uniform entry) after one warm-up call, host clock around call + synchronise; figures "
                     "are the median over the processes, min / max their spread",
           "noiseless_against_parent": {"uniform_fitted": against_parent(lambda r: r["uniform"]["fitted"]),
                                        "uniform_koff50": against_parent(lambda r: r["uniform"]["koff50"]),
                                        f"mapped_T{MAPPED_T}": against_parent(lambda r: r["mapped"])},
           "noise_on_against_off": {}}
    for T in NOISE_TRIALS:  # noqa: N806
        row = {}
        for form in ("planes", "no_planes"):
            off = summary([r["noise"][str(T)][form]["off"]["ms"] for r in runs["this"]])
            on = summary([r["noise"][str(T)][form]["on"]["ms"] for r in runs["this"]])
            row[form] = {"off": off, "on": on, "ratio_on_to_off": round(on["ms"] / off["ms"], 4),
                         "on_inside_off_min_max": bool(off["min_ms"] <= on["ms"] <= off["max_ms"]),
                         "checksums_differ": all(r["noise"][str(T)][form]["on"]["checksum"] != r["noise"][str(T)][form]["off"]["checksum"]
                                                 for r in runs["this"]),
                         "on_checksums": sorted({r["noise"][str(T)][form]["on"]["checksum"] for r in runs["this"]})}
        row["threads"] = T * GRID[0] * GRID[1]
        out["noise_on_against_off"][str(T)] = row
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent", default=None, help="session mode: a checkout of the parent commit with its own libnsof.so")
    ap.add_argument("--configs", default="uniform,mapped,noise", type=lambda s: s.split(","))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--uniform-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=280)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (session if args.parent else worker)(args)
