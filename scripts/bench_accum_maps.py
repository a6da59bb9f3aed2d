#!/usr/bin/env python3
"""Per-pixel parameter maps on the stream of scripts/bench_accum.py (BASELINE config 5: 1 M events/s, 1 ms slices, scheme 1,
active_v = -6, silent_v = 0) at 1280x720 and 3840x2160: slices/s of
  a  the fitted device (the compile-time instantiation)
  b  a uniform device that is not the fitted one (koff changed: the model in the kernel arguments)
  c  the device of b with every one of the 13 keys mapped to a constant plane (same states as b)
  d  the device of b with nsof.accumulator.variability_maps, 10 % spread on kon, koff, Ron, Roff
each through the every-pixel pass (dense=True) and the event-pixel update (dense=False), Accumulator.run over the stream.

Two ways to call it.
  worker   bench_accum_maps.py [--tree DIR] [--configs a,b,c,d]      one process, one JSON line.  --tree DIR measures the
           package under DIR (a checkout of another commit with its own libnsof.so; a tree without parameter maps takes
           --configs a,b, for which no map is passed).
  session  bench_accum_maps.py --parent DIR [--rounds 3] [--out profiles/accum_param_maps.json]
           starts workers alternately -- parent at a and b, this tree at every config -- `rounds` times in fresh processes and
           writes the medians over the rounds with their min-max spread, this tree's a and b against the parent's (the
           branch's median against the parent's min-max widened by that spread once more), and c / b and d / b.

Timing: the host clock around calls that end in a device synchronise; every (size, route, config) is warmed up by one untimed
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
SIZES = ((1280, 720), (3840, 2160))
ROUTES = ("every_pixel", "event_pixel")
SPREAD_KEYS = ("kon", "koff", "Ron", "Roff")
# what a mapped accumulator moves on top of the uniform one (float32 planes written once by the set-up kernel)
BYTES = {
    "event_pixel": "12 B (ka, s, b of the active drive) per listed pixel per group of up to 32 slices, on top of the 20 B the "
                   "uniform update moves for it (list 4, mask 4 + 4, w 4 + 4)",
    "every_pixel": "12 B per DRIVEN pixel per group of up to 64 slices (idle pixels load nothing), on top of the 16-20 B/px the "
                   "uniform pass moves for every pixel; with silent_v outside some pixel's dead zone 24 B for every pixel per "
                   "group (both drives), and 8 B/px (Ron, neg_lam) for a fused mode-0 frame",
}


def stream(np, W, H, n=1_000_000):  # noqa: N803
    rng = np.random.default_rng(5)                      # the stream of scripts/bench_accum.py, folded onto the sensor
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    k = int(0.3 * n)
    t = np.sort(rng.integers(0, 1_000_000, n)).astype(np.int64)
    drift = (t[:k] * 600e-6).astype(np.int64)
    x[:k] = (rng.integers(0, 400, k) + drift) % W
    y[:k] = rng.integers(0, 300, k) + H // 3
    p = rng.integers(0, 2, n)
    return x.astype(np.int16), y.astype(np.int16), p.astype(np.int8), t


def worker(a):
    root = os.path.abspath(a.tree)
    sys.path[:0] = [root, os.path.join(root, "neuromorphic-spatiotemporal-optical-flow_amd")]
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import nsof
    from nsof import accumulator as A  # noqa: N812
    ctx = nsof.Context(0)
    other = dict(A.PARAMS, koff=50.0)
    out = {"tree": root, "lib": nsof._lib.LIB_PATH, "reps": a.reps, "window_s": a.window, "sizes": {}}

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

    for W, H in SIZES:  # noqa: N806
        x, y, p, t = stream(np, W, H)
        idx = A.slice_index_array(t, 1000)
        n_sl = len(idx) - 1
        size = out["sizes"][f"{W}x{H}"] = {"slices": n_sl, "routes": {r: {} for r in ROUTES}}
        for cfg in a.configs:
            kw = {}
            if cfg != "a":
                kw["params"] = other
            if cfg == "c":
                kw["param_maps"] = {k: np.full((H, W), other[k], np.float32) for k in A._PARAM_KEYS}
            if cfg == "d":
                kw["param_maps"] = A.variability_maps(H, W, {k: 0.1 for k in SPREAD_KEYS}, other, seed=1)
            for route in ROUTES:
                acc = A.Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx, dense=route == "every_pixel", **kw)
                acc.set_events(x, y, p, t, idx)
                res = timed(lambda: acc.run(0, n_sl), n_sl)   # noqa: B023
                acc.reset()                                      # one run from the initial state: what the result is compared by
                acc.run(0, n_sl)
                ctx.synchronize()
                res["checksum"] = float(acc.w(0).astype("float64").sum())
                size["routes"][route][cfg] = res
                acc.close()
    ctx.close()
    print(json.dumps(out))


def session(a):
    me = os.path.abspath(__file__)

    def run(tree, configs):
        cmd = [sys.executable, me, "--tree", tree, "--configs", ",".join(configs), "--reps", str(a.reps), "--window", str(a.window)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, check=True)
        return json.loads(r.stdout.strip().splitlines()[-1])
    runs = {"parent": [], "this": []}
    for _ in range(a.rounds):                            # alternating: other work shares the machine
        runs["parent"].append(run(a.parent, ["a", "b"]))
        runs["this"].append(run(HERE, a.configs))

    def summary(rs, size, route, cfg):
        v = [r["sizes"][size]["routes"][route][cfg]["slices_per_s"] for r in rs]
        return {"slices_per_s": statistics.median(v), "min": min(v), "max": max(v), "per_process": v,
                "checksums": sorted({r["sizes"][size]["routes"][route][cfg]["checksum"] for r in rs})}
    out = {"workload": "1e6 events over 1 s, 1 ms slices, scheme 1, active_v=-6, silent_v=0, Accumulator.run over the 1000 slices; "
                       "a fitted device, b uniform with koff=50, c = b with all 13 keys as constant planes, d = b with 10 % spread "
                       "on " + ", ".join(SPREAD_KEYS),
           "method": f"{a.rounds} alternating fresh processes per tree; per process the median of {a.reps} windows of >= "
                     f"{a.window} s after one warm-up call; figures are the median over the processes, min / max their spread",
           "extra_bytes_of_a_mapped_accumulator": BYTES, "parent": {}, "this": {}, "unchanged_paths_vs_parent": {},
           "mapped_over_uniform": {}}
    for size in (f"{w}x{h}" for w, h in SIZES):
        for key in ("parent", "this", "unchanged_paths_vs_parent", "mapped_over_uniform"):
            out[key][size] = {r: {} for r in ROUTES}
        for route in ROUTES:
            for cfg in ("a", "b"):
                out["parent"][size][route][cfg] = summary(runs["parent"], size, route, cfg)
            for cfg in a.configs:
                out["this"][size][route][cfg] = summary(runs["this"], size, route, cfg)
            for cfg in ("a", "b"):
                par, one = out["parent"][size][route][cfg], out["this"][size][route][cfg]
                spread = par["max"] - par["min"]
                out["unchanged_paths_vs_parent"][size][route][cfg] = {
                    "branch_median": one["slices_per_s"], "parent_min": par["min"], "parent_max": par["max"],
                    "accepted_from": round(par["min"] - spread, 1), "accepted_to": round(par["max"] + spread, 1),
                    "ratio_to_parent_median": round(one["slices_per_s"] / par["slices_per_s"], 4),
                    "not_slower": bool(one["slices_per_s"] >= par["min"] - spread),
                    "inside": bool(par["min"] - spread <= one["slices_per_s"] <= par["max"] + spread),
                    "same_checksum": one["checksums"] == par["checksums"]}
            b = out["this"][size][route]["b"]
            for cfg in ("c", "d"):
                if cfg in a.configs:
                    m = out["this"][size][route][cfg]
                    out["mapped_over_uniform"][size][route][f"{cfg}/b"] = round(m["slices_per_s"] / b["slices_per_s"], 4)
            if "c" in a.configs:
                out["mapped_over_uniform"][size][route]["c_same_checksum_as_b"] = out["this"][size][route]["c"]["checksums"] == b["checksums"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fp:
            fp.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--parent", default=None, help="session mode: a checkout of the parent commit with its own libnsof.so")
    ap.add_argument("--configs", default="a,b,c,d", type=lambda s: s.split(","))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.25)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=280)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (session if args.parent else worker)(args)
