#!/usr/bin/env python3
"""A/B of two libnsof builds on the host-pointer work-list pipeline (nsof_farneback_px_batch) and the gated ROI sequence:
alternating fresh processes, the parent's library chosen by NSOF_LIB, median [min-max] per figure and whether the new
median lies inside the parent's own min-max.

Per round and library: ``bench.py`` (headline, e2e record, config3 record) and ``scripts/e2e_probe.py`` at its default size
(the faster of its two repetitions).  The first child that fails or runs out of time ends the run.

    python scripts/ab_pipe.py --parent PATH/libnsof_parent.so --rounds 6 --out profiles/pipe_refactor.json
    (--resume FILE: continue a run whose earlier rounds FILE holds)
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--no-fast-leg",
         "--no-param-legs", "--cpu-sample", "0"]
PROBE = [sys.executable, os.path.join(ROOT, "scripts", "e2e_probe.py")]


def child(cmd, lib, limit):
    env = dict(os.environ, NSOF_SKIP_BUILD="1")
    env.pop("NSOF_LIB", None)
    if lib:
        env["NSOF_LIB"] = lib
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd[1:3])} (NSOF_LIB={lib}) left with {r.returncode}:\n{r.stderr[-2000:]}")
    return r.stdout


def figures(lib):
    d = json.loads(child(BENCH, lib, 400).strip().splitlines()[-1])
    out = {"headline_pairs_per_s": d["value"], "e2e_pairs_per_s": d["e2e"]["value"],
           "e2e_pageable_outputs_pairs_per_s": d["e2e"]["pageable_outputs_pairs_per_s"],
           "e2e_one_call_per_pair_pairs_per_s": d["e2e"]["one_call_per_pair_pairs_per_s"]}
    for name, s in d["config3"]["streams"].items():
        out[f"config3_{name}_flow_ms"] = s["flow_ms"]
    if d.get("parity_ok") is False:
        raise SystemExit(f"bench.py (NSOF_LIB={lib}): parity_ok is false")
    reps = [float(x) for x in re.findall(r"rep \d+: ([0-9.]+) pairs/s", child(PROBE, lib, 200))]
    out["e2e_probe_pairs_per_s"] = max(reps)
    return out


def summary(runs):
    table = {}
    for key in runs["parent"][0]:
        row = {}
        for tree in ("parent", "new"):
            v = [r[key] for r in runs[tree]]
            row[tree] = {"median": statistics.median(v), "min": min(v), "max": max(v), "values": v}
        row["new_median_inside_parent_range"] = row["parent"]["min"] <= row["new"]["median"] <= row["parent"]["max"]
        table[key] = row
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="the parent commit's libnsof.so")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", required=True)
    ap.add_argument("--resume", default=None)
    args = ap.parse_args()
    runs = {"parent": [], "new": []}
    if args.resume:
        with open(args.resume) as f:
            runs = json.load(f)["runs"]
    for k in range(args.rounds):
        for tree, lib in (("parent", os.path.abspath(args.parent)), ("new", None)):
            runs[tree].append(figures(lib))
            print(f"round {k} {tree}: {runs[tree][-1]}", flush=True)
        with open(args.out, "w") as f:   # after every round: what has been measured survives a later failure
            json.dump({"_doc": __doc__.split("\n\n")[0], "command": "bench.py " + " ".join(BENCH[2:]) + "; scripts/e2e_probe.py",
                       "rounds": len(runs["new"]), "figures": summary(runs), "runs": runs}, f, indent=1)
    for key, row in summary(runs).items():
        p, n = row["parent"], row["new"]
        print(f"{key:45s} parent {p['median']:9.2f} [{p['min']:.2f}-{p['max']:.2f}]  new {n['median']:9.2f} "
              f"[{n['min']:.2f}-{n['max']:.2f}]  inside: {row['new_median_inside_parent_range']}")


if __name__ == "__main__":
    main()
