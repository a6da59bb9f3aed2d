#!/usr/bin/env python3
"""Monte-Carlo trials of the frame-driven gating array in one launch (nsof_accum_frames_f64_maps_dev): the grasp grid, 24
columns x 13 rows, 100 compressed frames, n_sub_steps 1000, 10 % spread on kon, koff, Ron, Roff
(nsof.accumulator.variability_maps, float64 planes), T in {1, 16, 256, 1024} trials.  Reported per T: time per launch
(plane upload included: it is part of the call) and trials/s; for T = 16 also the time of 16 sequential
simulate_frames_dev(params=...) calls -- the code before maps existed, what a user would otherwise do; and the uniform entry
(simulate_frames_dev without maps; the fitted device and one with koff = 50) on the parent commit and on this tree.

Two ways to call it.
  worker   bench_frames_trials.py [--tree DIR] [--configs uniform,trials]      one process, one JSON line.  --tree DIR measures
           the package under DIR (a checkout of another commit with its own libnsof.so; a tree without frame maps takes
           --configs uniform).  --configs host (no session runs it) times the host entry, simulate_frames on host arrays, on
           the same case.
  session  bench_frames_trials.py --parent DIR [--rounds 3] [--out profiles/frames_trials.json]
           starts workers alternately (the order swapped every round) -- parent at `uniform`, this tree at both -- `rounds`
           times in fresh processes and writes
           the medians over the processes with their min-max spread, and this tree's uniform entry against the parent's own
           min-max spread.

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
TRIALS = (1, 16, 256, 1024)
SPREAD_KEYS = ("kon", "koff", "Ron", "Roff")


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
    out = {"tree": root, "lib": nsof._lib.LIB_PATH, "reps": a.reps}

    def timed(call, reps=None):
        call()                                           # warm-up: allocations, code objects
        ctx.synchronize()
        ts = []
        for _ in range(reps or a.reps):
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
        return {"ms": round(1e3 * statistics.median(ts), 3), "min_ms": round(1e3 * min(ts), 3), "max_ms": round(1e3 * max(ts), 3)}

    def checksum(res):
        ctx.synchronize()
        return float(res[2].sum().item())

    if "uniform" in a.configs:
        out["uniform"] = {}
        for name, params in (("fitted", None), ("koff50", other)):
            r = timed(lambda: A.simulate_frames_dev(frames, n_sub_steps=N_SUB, ctx=ctx, params=params), a.uniform_reps)   # noqa: B023
            r["checksum"] = checksum(A.simulate_frames_dev(frames, n_sub_steps=N_SUB, ctx=ctx, params=params))
            out["uniform"][name] = r
    if "trials" in a.configs:
        out["trials"] = {}
        sigma = {k: 0.1 for k in SPREAD_KEYS}
        for T in TRIALS:  # noqa: N806
            maps = A.variability_maps(GRID[0], GRID[1], sigma, other, seed=1, trials=T, dtype=np.float64)
            r = timed(lambda: A.simulate_frames_dev(frames, n_sub_steps=N_SUB, ctx=ctx, params=other, param_maps=maps))   # noqa: B023
            r["trials_per_s"] = round(T / (r["ms"] * 1e-3), 1)
            r["threads"] = T * GRID[0] * GRID[1]
            got = A.simulate_frames_dev(frames, n_sub_steps=N_SUB, ctx=ctx, params=other, param_maps=maps)
            r["checksum"] = checksum(got)
            if T == 16:   # the same 16 studies as 16 uniform calls: per call the device of that trial's first cell
                devices = [dict(other, **{k: float(maps[k][t, 0, 0]) for k in SPREAD_KEYS}) for t in range(T)]
                s = timed(lambda: [A.simulate_frames_dev(frames, n_sub_steps=N_SUB, ctx=ctx, params=p) for p in devices])   # noqa: B023
                seq = [A.simulate_frames_dev(frames, n_sub_steps=N_SUB, ctx=ctx, params=p)[2] for p in devices]
                ctx.synchronize()
                s["first_cells_equal_the_mapped_run"] = all(bool(torch.equal(seq[t][:, 0, 0], got[2][t, :, 0, 0])) for t in range(T))
                s["speedup_of_one_launch"] = round(s["ms"] / r["ms"], 2)
                r["sequential_uniform_calls"] = s
            out["trials"][str(T)] = r
    if "host" in a.configs:   # the host entry on the same case (simulate_frames on host arrays: copies both ways around the launch)
        out["host"] = {}
        h = frames.cpu().numpy()
        for name, params in (("fitted", None), ("koff50", other)):
            r = timed(lambda: A.simulate_frames(h, n_sub_steps=N_SUB, ctx=ctx, params=params), a.uniform_reps)   # noqa: B023
            r["checksum"] = float(A.simulate_frames(h, n_sub_steps=N_SUB, ctx=ctx, params=params)[1].sum())
            out["host"][name] = r
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
            runs[which].append(run(a.parent, ["uniform"]) if which == "parent" else run(HERE, ["uniform", "trials"]))

    def summary(values):
        return {"ms": statistics.median(values), "min_ms": min(values), "max_ms": max(values), "per_process": values}
    out = {"workload": f"grid {GRID[1]}x{GRID[0]} (grasp), {N_FRAMES} frames, n_sub_steps {N_SUB}, dt 5e-4, th1 0.7, th2 1.5; uniform random "
                       "frames (every pair drives every cell); trials: params with koff=50, 10 % spread on " + ", ".join(SPREAD_KEYS),
           "method": f"{a.rounds} alternating fresh processes per tree; per process the median of {a.reps} timed calls "
                     f"({a.uniform_reps} for the uniform entry) after one warm-up call, host clock around call + synchronise; figures are the median over the processes, min / max "
                     "their spread",
           "bytes": "per (trial, cell): 8 B per mapped key plus 16 B (lambda, r0) uploaded once per call; 8 B x (2 n_frames - 1) "
                    "+ 8 B written (res, current, w); the frames are read by every trial (8 B x n_frames per thread, L2 hits)",
           "uniform_entry": {}, "trials": {}}
    for name in ("fitted", "koff50"):
        par = summary([r["uniform"][name]["ms"] for r in runs["parent"]])
        one = summary([r["uniform"][name]["ms"] for r in runs["this"]])
        out["uniform_entry"][name] = {
            "parent": par, "this": one, "ratio_to_parent_median": round(one["ms"] / par["ms"], 4),
            "inside_parent_min_max": bool(par["min_ms"] <= one["ms"] <= par["max_ms"]),
            "not_slower_than_parent_max": bool(one["ms"] <= par["max_ms"]),
            "same_checksum": sorted({r["uniform"][name]["checksum"] for r in runs["parent"]})
            == sorted({r["uniform"][name]["checksum"] for r in runs["this"]})}
    for T in TRIALS:  # noqa: N806
        rs = [r["trials"][str(T)] for r in runs["this"]]
        t = summary([r["ms"] for r in rs])
        t.update(threads=rs[0]["threads"], trials_per_s=round(T / (t["ms"] * 1e-3), 1), checksums=sorted({r["checksum"] for r in rs}))
        if T == 16:
            s = summary([r["sequential_uniform_calls"]["ms"] for r in rs])
            s["speedup_of_one_launch"] = round(s["ms"] / t["ms"], 2)
            s["first_cells_equal_the_mapped_run"] = all(r["sequential_uniform_calls"]["first_cells_equal_the_mapped_run"] for r in rs)
            t["sequential_uniform_calls"] = s
        out["trials"][str(T)] = t
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent", default=None, help="session mode: a checkout of the parent commit with its own libnsof.so")
    ap.add_argument("--configs", default="uniform,trials", type=lambda s: s.split(","))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--uniform-reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=280)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (session if args.parent else worker)(args)
