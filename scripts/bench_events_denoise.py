#!/usr/bin/env python3
"""The background-activity filter (``nsof.events_denoise_dev``); prints one JSON line.

    python scripts/bench_events_denoise.py [--frames 64 --reps 10 --kernel-stats CSV --parent-lib PATH --out profiles/events_denoise.json]

Input: the stream of scripts/bench_events_sensor.py's "noise" path -- --frames frames of 1080p drifting texture 33333 us
apart, threshold 10 grey levels, ``ref="first"``, linear stamps, 1 Hz of background activity -- left in HBM by the generator.

  call      after a warm-up, --reps rounds of ``events_denoise_dev`` as a user makes it (both entries, output allocation,
            ``bounds=frame_bounds``) and of its two entries alone through ctypes on preallocated outputs, each between two
            device events on the context's stream: median and min-max in ms, events per second of the call's median.
  sort      with --kernel-stats (the kernel_stats.csv of a separate ``rocprofv3 --kernel-trace --stats`` run of
            ``--trace``, scripts/prof_py_kernels.sh): the share of the rocprim kernels in the kernel time of a call, and every
            kernel's share.
  numpy     the NumPy restatement of the sorted-segment formulation (tests/events_denoise_ref.py) on the events of the first
            --ref-frames frames of the same stream (a prefix of a stream is a first chunk: same decisions), its time, and
            whether keep and last are equal to the device's on that prefix.
  shares    two kept shares that need no labels, at dt_us 1000, 5000 and 20000: of the stream of a constant video with noise
            only (every event is noise: the false-positive rate) and of the noiseless stream of the drifting texture (signal
            retention).
  parent    with --parent-lib (libnsof.so of the parent commit, built beside this one), as in scripts/bench_events_sensor.py:
            the mark entry and the compact entry of both libraries, each library on a fresh context and outputs of its own,
            the two alternating within every round and the one that goes first changing from round to round.  The run
            asserts that both give the same keep, bounds, kept stream and last; ``within_parent_range``: the new median of an
            entry lies inside the parent's min-max of this session (or below it).
--trace runs the call --reps times after the warm-up and nothing else.
Not measured: see "not_measured" in the record."""
import argparse
import ctypes as C
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd"), os.path.join(ROOT, "tests")]
H, W = 1080, 1920
FRAME_US = 33333
THRESHOLD = 10.0
NOISE = dict(seed=1, rate_hz=1)
FILTER = dict(dt_us=5000, radius=1, min_support=1, same_polarity=False, include_self=False)
DT_US = (1000, 5000, 20000)


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def kernel_shares(path):
    """The filter's kernels in a kernel_stats.csv: k_ed_*, its k_ev_scan and the keys-only radix sort (the generator's sort carries values)."""
    ns = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "k_ed_" in name or "k_ev_scan<false>" in name:   # (k_ev_scan<true> is the generator's)
            key = "k_e" + name.split("::k_e")[1].split("(")[0].split("<")[0]
        elif "rocprim" in name and "radix_sort" in name and "unsigned int const*" not in name:
            key = "rocprim_radix_sort"
        else:
            continue
        ns[key] = ns.get(key, 0.0) + float(r["TotalDurationNs"])
    total = sum(ns.values())
    shares = {k: round(v / total, 4) for k, v in sorted(ns.items(), key=lambda kv: -kv[1])}
    return {"sort_share_of_kernel_time": shares.get("rocprim_radix_sort"), "kernel_shares": shares}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-frames", type=int, default=8, help="the NumPy restatement runs on the events of this many frames")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats.csv of a rocprofv3 run of --trace")
    ap.add_argument("--parent-lib", default=None, help="libnsof.so of the parent commit, for the alternating entry-by-entry check")
    ap.add_argument("--trace", action="store_true", help="the call --reps times and nothing else")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import _lib, synth
    from events_denoise_ref import denoise_sorted
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n = a.frames
    times = np.arange(n, dtype=np.int64) * FRAME_US
    frames = torch.from_numpy(synth.make_sequence(7, n, H, W, pad=192)).to(dev)
    gen = dict(threshold=THRESHOLD, ref="first", timestamps="linear", ctx=ctx)
    ev = nsof.events_from_frames_dev(frames, times, noise=NOISE, **gen)
    ctx.synchronize()
    xs = tuple(ev[k] for k in "xypt")
    total = int(ev["frame_bounds"][-1])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def call():
        return nsof.events_denoise_dev(*xs, (H, W), bounds=ev["frame_bounds"], ctx=ctx, **FILTER)

    res = call()   # warm-up: the workspace
    ctx.synchronize()
    n_kept = res["n_kept"]
    if a.trace:
        for _ in range(a.reps):
            call()
        ctx.synchronize()
        print(json.dumps({"bench": "events_denoise", "trace_reps": a.reps, "frames": n, "events": total}))
        ctx.close()
        return

    b_in = ev["frame_bounds"]

    def entries(lib, ptr):
        """The two entries of ``lib`` alone on its context ``ptr`` -> (mark, compact, their preallocated outputs: keep, x, y, p, t,
        last, and the host bounds)."""
        keep = torch.empty(total, dtype=torch.uint8, device=dev)
        out = [torch.empty(n_kept, dtype=v.dtype, device=dev) for v in xs]
        last = torch.empty((1, H, W), dtype=torch.int64, device=dev)
        b_out, kept = np.zeros(n + 1, np.int64), C.c_int64()
        head = (ptr, *(v.data_ptr() for v in xs), total, H, W)

        def mark():
            rc = lib.nsof_events_denoise_mark_dev(*head, FILTER["dt_us"], FILTER["radius"], FILTER["min_support"], 0, 0, None,
                                                  b_in.ctypes.data, n + 1, keep.data_ptr(), C.byref(kept), b_out.ctypes.data)
            assert rc == 0 and kept.value == n_kept, (rc, kept.value)

        def compact():
            rc = lib.nsof_events_denoise_compact_dev(*head, 0, None, keep.data_ptr(), n_kept, *(v.data_ptr() for v in out), last.data_ptr())
            assert rc == 0, rc
        return mark, compact, (keep, *out, last), b_out

    mark, compact, (keep, *out, last), b_out = entries(ctx._lib, ctx.ptr)
    torch.cuda.synchronize(dev)
    ms = {"call": [], "mark_entry": [], "compact_entry": []}
    for _ in range(a.reps):
        t_ms, r = timed(call)
        ms["call"].append(t_ms)
        del r
        ms["mark_entry"].append(timed(mark)[0])
        ms["compact_entry"].append(timed(compact)[0])
    ctx.synchronize()
    same_entries = all(torch.equal(o, res[k]) for o, k in zip(out, "xypt")) and torch.equal(keep, res["keep"]) and \
        torch.equal(last, res["last"]) and np.array_equal(b_out, res["bounds"])
    line = {"bench": "events_denoise", "frames": n, "frame_hw": [H, W], "frame_us": FRAME_US, "threshold_grey": THRESHOLD, "ref": "first",
            "timestamps": "linear", "noise_hz": NOISE["rate_hz"], "filter": FILTER, "reps": a.reps, "events": total, "kept": n_kept,
            "kept_share": round(n_kept / total, 4), "entries_equal_the_call": bool(same_entries)}
    line.update({k: spread(v) for k, v in ms.items()})
    line["events_per_s"] = round(total / (line["call"]["median_ms"] * 1e-3))
    if a.kernel_stats:
        line.update(kernel_shares(a.kernel_stats))
    if a.parent_lib:
        libs = {"new": ctx._lib, "parent": C.CDLL(os.path.abspath(a.parent_lib))}
        for name in ("nsof_create", "nsof_destroy", "nsof_set_stream", "nsof_events_denoise_mark_dev", "nsof_events_denoise_compact_dev"):
            fn = getattr(libs["parent"], name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        ptrs, calls, results = {}, {}, {}
        for which in ("parent", "new"):   # a fresh context of each library: the one above has the workspace of the calls it ran
            ptrs[which] = C.c_void_p()
            assert libs[which].nsof_create(0, C.byref(ptrs[which])) == 0
            assert libs[which].nsof_set_stream(ptrs[which], C.c_void_p(stream.cuda_stream)) == 0
            calls[which, "mark_entry"], calls[which, "compact_entry"], *results[which] = entries(libs[which], ptrs[which])
            for v in results[which][0]:
                v.zero_()
            torch.cuda.synchronize(dev)
            calls[which, "mark_entry"]()   # warm-up; what the two libraries wrote is compared below
            calls[which, "compact_entry"]()
            torch.cuda.synchronize(dev)
        assert all(torch.equal(v, w) for v, w in zip(results["new"][0], results["parent"][0])), "keep, the kept stream or last differ"
        assert np.array_equal(results["new"][1], results["parent"][1]), "the bounds differ"
        pm = {key: [] for key in calls}
        for r in range(a.reps):
            for what in ("mark_entry", "compact_entry"):
                for which in (("parent", "new"), ("new", "parent"))[r % 2]:   # who goes first changes every round
                    pm[which, what].append(timed(calls[which, what])[0])
        line["vs_parent"] = {"same_keep_bounds_stream_and_last": True}
        for what in ("mark_entry", "compact_entry"):
            new, par = spread(pm["new", what]), spread(pm["parent", what])
            line["vs_parent"][what] = {"new": new, "parent": par, "within_parent_range": new["median_ms"] <= par["max_ms"]}
        for which in ptrs:
            libs[which].nsof_destroy(ptrs[which])

    # the NumPy restatement on a prefix of the same stream
    m = int(ev["frame_bounds"][min(a.ref_frames, n)])
    host = [v[:m].cpu().numpy() for v in xs]
    t0 = time.perf_counter()
    keep_ref, last_ref = denoise_sorted(*host, H, W, **FILTER)
    numpy_s = time.perf_counter() - t0
    pre = nsof.events_denoise_dev(*(v[:m] for v in xs), (H, W), ctx=ctx, **FILTER)
    ctx.synchronize()
    line["numpy_restatement"] = {"frames": min(a.ref_frames, n), "events": m, "seconds": round(numpy_s, 3),
                                 "events_per_s": round(m / numpy_s),
                                 "keep_equal": bool(np.array_equal(pre["keep"].cpu().numpy(), keep_ref)),
                                 "last_equal": bool(np.array_equal(pre["last"].cpu().numpy(), last_ref)),
                                 "prefix_of_the_full_call_equal": bool(torch.equal(pre["keep"], res["keep"][:m]))}
    del pre, res, keep, out, last, host

    # the two kept shares that need no labels
    flat = torch.full((n, H, W), 128, dtype=torch.uint8, device=dev)
    only_noise = nsof.events_from_frames_dev(flat, times, noise=NOISE, **gen)
    clean = nsof.events_from_frames_dev(frames, times, **gen)
    ctx.synchronize()
    shares = {"noise_only_events": int(only_noise["frame_bounds"][-1]), "clean_events": int(clean["frame_bounds"][-1]), "dt_us": {}}
    for dt in DT_US:
        kw = dict(FILTER, dt_us=dt)
        fp = nsof.events_denoise_dev(*(only_noise[k] for k in "xypt"), (H, W), ctx=ctx, **kw)["n_kept"]
        keep_n = nsof.events_denoise_dev(*(clean[k] for k in "xypt"), (H, W), ctx=ctx, **kw)["n_kept"]
        ctx.synchronize()
        shares["dt_us"][str(dt)] = {"false_positive_rate": round(fp / max(shares["noise_only_events"], 1), 6),
                                    "signal_retention": round(keep_n / max(shares["clean_events"], 1), 6)}
    line["kept_shares"] = shares
    line["not_measured"] = ["hardware counters", "frame sizes other than 1080p", "radius 2, min_support above 1, same_polarity, include_self",
                            "chunked runs and a given last plane", "the sequential NumPy walk on the whole stream (minutes)",
                            "the compact entry without last_out", "labelled data sets"]
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
