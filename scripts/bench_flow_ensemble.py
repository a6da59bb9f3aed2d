#!/usr/bin/env python3
"""Flow statistics over Monte-Carlo trials (``nsof.flow_ensemble_dev``, ``nsof.events_flow_variability_dev``); prints one
JSON line.

    python scripts/bench_flow_ensemble.py [--trials 64 8 --reps 10 --pipeline-trials 16 --kernel-stats <kernel_stats.csv>]
                                          [--out profiles/flow_ensemble.json]

  kernel:    seeded float32 flows [T][1][1080][1920][2] (normal, sigma 5 px) against a reference field, T = --trials.  Per T,
             after a warm-up of both, --reps rounds that alternate
               device   one ``flow_ensemble_dev`` call that starts the state (``start``) and one that continues it
                        (``continue``: the state is read as well as written), each between two device events on the
                        context's stream;
               torch    the same statistics as float64 torch expressions on the same tensors -- what a user writes
                        without the entry -- between two device events;
             median and min-max of each in ms; the bytes the algorithm needs (flows 8 T H W, reference 8 H W, state 48 H W
             written and, continuing, 48 H W read; the workgroup partials are left out: 16 B per 512 pixels and trial) and
             their rate as a share of the 8 TB/s peak at the median; whether the two agree (sum, sq, aee to 1e-12
             relative to the largest magnitude, epe2_max and the counts exactly).
  pipeline:  ``events_flow_variability_dev`` on the config-3 stream (1280 x 720, ``synth.make_events(2024)``, 1000 slices,
             30 frames) with 10 % spread on koff and --pipeline-trials trials: wall time of a second run and its split
             into nominal run, trial accumulator, trial flows and ensemble reduction (host clock around stages that end in
             a synchronise).
With --kernel-stats (the kernel_stats.csv of a separate ``rocprofv3 --kernel-trace --stats`` run of this script with
--trace) the average time of the two kernels follows.  --trace runs the device calls of the kernel leg and nothing else."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]
HBM_PEAK = 8e12
H, W = 1080, 1920
TAU = 3.0


def model_bytes(trials, accumulate):
    return (8 * trials + 8 + 48 * (2 if accumulate else 1)) * H * W


def torch_stats(torch, flows, ref, tau):
    d = flows.to(torch.float64) - ref.to(torch.float64)
    du, dv = d[..., 0], d[..., 1]
    uu, vv = du * du, dv * dv
    e2 = uu + vv
    return dict(sum=d.sum(0), sq=torch.stack((uu.sum(0), vv.sum(0), (du * dv).sum(0)), -1), epe2_max=e2.amax(0),
                aee=e2.sqrt().mean((2, 3)), outliers=(e2 > tau * tau).sum((2, 3)), nonfinite=(~(e2 < float("inf"))).sum((2, 3)))


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def kernel_times(path):
    """kernel -> calls and average / min / max us over ALL launches of the traced run (every T of --trials, starting and
    continuing) from a rocprofv3 kernel_stats.csv."""
    out = {}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            for frag, key in (("k_flow_ensemble_finish", "k_flow_ensemble_finish"), ("k_flow_ensemble<", "k_flow_ensemble")):
                if frag in row["Name"]:
                    out[key] = {"calls": int(row["Calls"]), **{k + "_us": round(float(row[c]) / 1e3, 2) for k, c in
                                                               (("avg", "AverageNs"), ("min", "MinNs"), ("max", "MaxNs"))}}
                    break
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, nargs="+", default=[64, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pipeline-trials", type=int, default=16)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import torch

    import nsof
    from nsof import synth
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    stream = torch.cuda.Stream(dev)   # one stream for the library and torch: device events bracket both formulations
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(2024)
    line = {"bench": "flow_ensemble", "field_hw": [H, W], "fields": 1, "reps": a.reps, "tau": TAU, "kernel": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    for n_t in a.trials:
        flows = torch.randn((n_t, 1, H, W, 2), generator=gen, device=dev, dtype=torch.float32) * 5
        ref = torch.randn((1, H, W, 2), generator=gen, device=dev, dtype=torch.float32)
        state = nsof.flow_ensemble_dev(flows, ref, TAU, ctx=ctx)
        if a.trace:
            for _ in range(a.reps):
                nsof.flow_ensemble_dev(flows, ref, TAU, ctx=ctx)
                nsof.flow_ensemble_dev(flows, ref, TAU, state=state, ctx=ctx)
            ctx.synchronize()
            continue
        want = torch_stats(torch, flows, ref, TAU)   # warm-up of the torch side, and the comparison
        torch.cuda.synchronize(dev)
        agree = {}
        for k in ("sum", "sq", "aee"):
            agree[k] = bool(((state[k] - want[k]).abs().max() <= 1e-12 * want[k].abs().max()).item())
        for k in ("epe2_max", "outliers", "nonfinite"):
            agree[k] = bool(torch.equal(state[k], want[k].to(state[k].dtype)))
        del want
        ms = {"start": [], "continue": [], "torch": []}
        for _ in range(a.reps):
            ms["start"].append(timed(lambda: nsof.flow_ensemble_dev(flows, ref, TAU, ctx=ctx))[0])
            ms["continue"].append(timed(lambda: nsof.flow_ensemble_dev(flows, ref, TAU, state=state, ctx=ctx))[0])
            t_ms, out = timed(lambda: torch_stats(torch, flows, ref, TAU))
            ms["torch"].append(t_ms)
            del out
        entry = {k: spread(v) for k, v in ms.items()}
        for k, acc in (("start", False), ("continue", True)):
            entry[k]["model_bytes"] = model_bytes(n_t, acc)
            entry[k]["hbm_share"] = round(model_bytes(n_t, acc) / (entry[k]["median_ms"] * 1e-3) / HBM_PEAK, 4)
        entry["torch_over_device"] = round(entry["torch"]["median_ms"] / entry["start"]["median_ms"], 2)
        entry["torch_peak_bytes"] = int(torch.cuda.max_memory_allocated(dev))
        entry["agree"] = agree
        line["kernel"][f"T={n_t}"] = entry
        del flows, ref, state
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats(dev)
    if a.trace:
        print(json.dumps({"bench": "flow_ensemble", "trace_reps": a.reps, "trials": a.trials}))
        return

    x, y, p, t = synth.make_events(2024)
    timings = {}
    for _ in range(2):   # the first run warms every shape up
        t0 = time.perf_counter()
        res = nsof.events_flow_variability_dev(x, y, p, t, (720, 1280), dict(koff=0.1), a.pipeline_trials, tau=TAU, ctx=ctx,
                                               timings=timings)
        wall = time.perf_counter() - t0
    line["pipeline"] = {"stream": "make_events(2024), 1280x720", "trials": a.pipeline_trials, "rel_sigma": {"koff": 0.1},
                        "frames": timings["frames"], "trial_chunk": timings["trial_chunk"], "wall_s": round(wall, 4),
                        **{k: round(timings[k], 4) for k in ("nominal_s", "trial_accumulator_s", "trial_flows_s", "ensemble_s")},
                        "aee_mean_px": round(float(res["aee"].mean().item()), 6),
                        "outlier_share": round(float(res["outliers"].double().mean().item()) / (720 * 1280), 6)}
    if a.kernel_stats:
        line["kernels_rocprofv3"] = kernel_times(a.kernel_stats)
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
