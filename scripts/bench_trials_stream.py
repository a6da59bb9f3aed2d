#!/usr/bin/env python3
"""What the resumable trial accumulator costs and moves: the 1280x720 stream of scripts/bench_accum_maps.py (1 M events over
1 s, 1 ms slices: 1000 slices), scheme 1, active_v = -6, silent_v = 0, T = 128 trials of identical devices that differ by
their cycle-to-cycle noise (c2c = dict(sigma=0.05, seed=1); no plane: the call is the staged stream and the kernels, not a
host pass over planes), block currents of 80 x 80 blocks after every 33rd slice.
  parent   nsof.simulate_trials_dev of the PARENT commit's tree (--parent DIR: a checkout with its own libnsof.so)
  oneshot  the same call on this tree (now: TrialAccumulator, one step, read-outs, close)
  chunks   this tree, nsof.TrialAccumulator created, stepped over the stream cut into 1, 2, 8 and 32 chunks of equal slice
           counts, read out (w, resistance) and closed: the whole of that timed, per chunk count; the checksums must agree
  surface  this tree, surface_u8_dev(mode="state") of all T trials into a dense [T][H][W] tensor, `launches` back to back
           between two synchronisations: T * H * W * (4 B in + 1 B out) over the time per launch, against 8 TB/s

Two ways to call it.
  worker   bench_trials_stream.py --what parent|oneshot|chunks|surface [--tree DIR]      one process, one JSON line
  session  bench_trials_stream.py --parent DIR [--rounds 3] [--out profiles/accum_trials_stream.json]
           starts the four kinds of worker alternately, `rounds` times in fresh processes, and writes the medians over the
           processes with their min-max spread, and whether the one-shot median lies inside the parent's min-max.  Nothing
           else is asserted: the per-chunk overhead and the surface rate are recorded.

Timing: the host clock around work that ends in a device synchronise; one untimed warm-up, then `reps` timed repetitions; a
process reports its median."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_accum_maps import stream  # noqa: E402

W, H, EVERY, MEMSIZE, TRIALS = 1280, 720, 33, 80, 128
NOISE = dict(sigma=0.05, seed=1)
CHUNKS = (1, 2, 8, 32)
FORMS = ("parent", "oneshot", "chunks", "surface")
HBM_PEAK = 8e12


def worker(a):
    root = os.path.abspath(a.tree)
    sys.path[:0] = [root, os.path.join(root, "neuromorphic-spatiotemporal-optical-flow_amd")]
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import nsof
    from nsof import accumulator as A  # noqa: N812
    ctx = nsof.Context(0)
    ev = stream(np, W, H)
    out = {"what": a.what, "tree": root, "lib": nsof._lib.LIB_PATH, "reps": a.reps, "trials": a.trials}

    def timed(call, reps=a.reps):
        got = call()                                      # warm-up: allocations, code objects
        ctx.synchronize()
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ctx.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return got, {"ms": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}

    def checksum(d):
        return [float(d[k].double().sum().item()) for k in ("w", "resistance", "block_current")]

    if a.what in ("parent", "oneshot"):
        got, t = timed(lambda: A.simulate_trials_dev(ev, None, 1, 1000, -6.0, 0.0, sensor_size=(H, W), snapshot_every=EVERY, memsize=MEMSIZE,
                                                     ctx=ctx, trials=a.trials, c2c=NOISE))
        out.update(t, checksum=checksum(got))
    else:
        import torch
        idx = A.slice_index_array(ev[3], 1000)
        n = len(idx) - 1

        def make():
            return A.TrialAccumulator(H, W, None, 1, "split", -6.0, 0.0, trials=a.trials, c2c=NOISE, snapshot_every=EVERY, memsize=MEMSIZE,
                                      ctx=ctx)
        if a.what == "chunks":
            def run(k):
                acc = make()
                try:
                    edges = [n * i // k for i in range(k + 1)]
                    cur = [acc.step(*ev, idx[lo:hi + 1]) for lo, hi in zip(edges, edges[1:])]
                    res = dict(w=acc.w_dev(), resistance=acc.resistance_dev(), block_current=torch.cat(cur, 2))
                    ctx.synchronize()
                    return res
                finally:
                    acc.close()
            out["slices"] = n
            for k in CHUNKS:
                got, t = timed(lambda k=k: run(k))
                out[f"chunks_{k}"] = dict(t, checksum=checksum(got))
        else:
            acc = make()
            acc.step(*ev, idx)
            frames = torch.empty((a.trials, H, W), dtype=torch.uint8, device=torch.device("cuda", ctx.device))
            torch.cuda.synchronize()

            def burst():
                for _ in range(a.launches):
                    acc.surface_u8_dev(frames, mode="state")
            _, t = timed(burst, max(a.reps, 5))
            moved = a.trials * H * W * 5
            per = {k: v / a.launches for k, v in t.items()}
            out.update(launches=a.launches, bytes_per_launch=moved, ms_per_launch=round(per["ms"], 4), min=round(per["min"], 4),
                       max=round(per["max"], 4), gb_per_s=round(moved / (per["ms"] * 1e-3) / 1e9, 1),
                       share_of_hbm_peak=round(moved / (per["ms"] * 1e-3) / HBM_PEAK, 4), checksum=float(frames.double().sum().item()))
            acc.close()
    ctx.close()
    print(json.dumps(out))


def session(a):
    me = os.path.abspath(__file__)

    def run(what):
        cmd = [sys.executable, me, "--what", what, "--reps", str(a.reps), "--trials", str(a.trials), "--launches", str(a.launches), "--tree",
               a.parent if what == "parent" else HERE]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, check=True)
        print(r.stdout.strip().splitlines()[-1], file=sys.stderr, flush=True)   # progress: a session takes minutes
        return json.loads(r.stdout.strip().splitlines()[-1])
    runs = {f: [] for f in FORMS}
    for _ in range(a.rounds):                            # alternating: other work shares the machine
        for what in FORMS:
            runs[what].append(run(what))

    def summary(rs, key=None, ms="ms"):
        rs = [r[key] if key else r for r in rs]
        v = [r[ms] for r in rs]
        return {"ms": statistics.median(v), "min": min(v), "max": max(v), "per_process": v,
                "checksums": sorted({json.dumps(r["checksum"]) for r in rs})}
    parent, oneshot = summary(runs["parent"]), summary(runs["oneshot"])
    chunks = {k: summary(runs["chunks"], f"chunks_{k}") for k in CHUNKS}
    surf = summary(runs["surface"], ms="ms_per_launch")
    moved = runs["surface"][0]["bytes_per_launch"]
    out = {"workload": f"1e6 events over 1 s on {W}x{H}, 1 ms slices, scheme 1, active_v=-6, silent_v=0, T = {a.trials} trials of identical "
                       f"devices with c2c = {NOISE}, block currents of {MEMSIZE}x{MEMSIZE} blocks after every {EVERY}rd slice",
           "method": f"{a.rounds} alternating fresh processes per form; per process one warm-up and the median of {a.reps} timed "
                     "repetitions, host clock around work that ends in a device synchronise; figures are the median over the "
                     "processes, min / max their spread",
           "parent": parent, "oneshot": oneshot,
           "oneshot_vs_parent": {"inside_parent_min_max": bool(parent["min"] <= oneshot["ms"] <= parent["max"]),
                                 "ratio_to_parent_median": round(oneshot["ms"] / parent["ms"], 4),
                                 "same_checksums": oneshot["checksums"] == parent["checksums"]},
           "chunks": {str(k): dict(v, over_one_chunk=round(v["ms"] / chunks[1]["ms"], 4),
                                   ms_per_extra_chunk=round((v["ms"] - chunks[1]["ms"]) / (k - 1), 4) if k > 1 else 0.0,
                                   same_checksums_as_one_chunk=v["checksums"] == chunks[1]["checksums"]) for k, v in chunks.items()},
           "surface_u8_all_trials": dict(surf, bytes_per_launch=moved, launches_per_burst=a.launches,
                                         gb_per_s=round(moved / (surf["ms"] * 1e-3) / 1e9, 1),
                                         share_of_8_tb_per_s=round(moved / (surf["ms"] * 1e-3) / HBM_PEAK, 4))}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=FORMS, default="oneshot")
    ap.add_argument("--parent", default=None, help="session mode: a checkout of the parent commit with its own libnsof.so")
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--trials", type=int, default=TRIALS)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=900)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (session if args.parent else worker)(args)
