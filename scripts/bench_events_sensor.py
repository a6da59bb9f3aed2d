#!/usr/bin/env python3
"""The event generator's sensor model (``nsof.events_from_frames_dev(refractory_us=, noise=)``); prints one JSON line.

    python scripts/bench_events_sensor.py [--frames 64 --reps 10 --parent-lib PATH --out profiles/events_sensor.json]

Input: that of scripts/bench_events_from_frames.py -- --frames frames of 1080p drifting texture 33333 us apart, threshold 10
grey levels, ``ref="first"``.

  paths    per timestamp mode, after a warm-up, --reps rounds that alternate four calls of ``events_from_frames_dev`` as a
           user makes them (count + emit entries, output allocation), each between two device events on the context's stream:
             plain        the default arguments (the plain entries and kernels)
             refractory   ``refractory_us=800`` alone (the walk against t_ok, no noise draw)
             noise        ``noise=dict(seed=1, rate_hz=1)`` alone (one Philox block per pixel and frame, no walk)
             both         the two together
           median and min-max of each in ms, the number of events of each stream, and ``over_plain`` = median / the plain
           median of the same mode.
  parent   with --parent-lib (libnsof.so of the parent commit, built beside this one): the count and emit entries of the
           plain pair and of the sensor pair (refractory time and noise together, both stamp modes), which both libraries
           export, called through ctypes on a fresh context of each library, the two libraries alternating within every round
           and the one that goes first changing from round to round.
           ``within_parent_range``: the new median of a call lies inside the parent's min-max of this session (or below
           it); ``same_stream_sums``: after every emit entry the two libraries' x, y, p, t, ref and t_ok add up alike.
           This is the check that a change of the kernels' code changed neither their results nor their time.
--trace MODE:PATH (say linear:both) runs that one call --reps times after the warm-up and nothing else, for a separate
``rocprofv3 --kernel-trace --stats`` run (scripts/prof_py_kernels.sh): the count kernel is one instantiation for all
sensor paths, so a trace of several would average them.
Not measured: hardware counters, frame sizes other than 1080p, rate planes (hot pixels), chunked runs, a given t_ok plane."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd"), os.path.join(ROOT, "tests")]
H, W = 1080, 1920
FRAME_US = 33333
THRESHOLD = 10.0
REFRACTORY_US = 800
NOISE = dict(seed=1, rate_hz=1)
PATHS = {"plain": {}, "refractory": dict(refractory_us=REFRACTORY_US), "noise": dict(noise=NOISE),
         "both": dict(refractory_us=REFRACTORY_US, noise=NOISE)}


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent-lib", default=None, help="libnsof.so of the parent commit, for the alternating entry-by-entry check")
    ap.add_argument("--trace", default=None, metavar="MODE:PATH", help="that call --reps times and nothing else")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import _lib, synth
    from events_from_frames_ref import units
    from events_sensor_ref import rate_q
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n = a.frames
    times = np.arange(n, dtype=np.int64) * FRAME_US
    frames = torch.from_numpy(synth.make_sequence(7, n, H, W, pad=192)).to(dev)
    line = {"bench": "events_sensor", "frames": n, "frame_hw": [H, W], "frame_us": FRAME_US, "threshold_grey": THRESHOLD, "ref": "first",
            "refractory_us": REFRACTORY_US, "noise_hz": NOISE["rate_hz"], "reps": a.reps, "modes": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def user(mode, kw):
        return nsof.events_from_frames_dev(frames, times, threshold=THRESHOLD, ref="first", timestamps=mode, ctx=ctx, **kw)

    calls = {(m, k): (lambda m=m, kw=kw: user(m, kw)) for m in ("frame", "linear") for k, kw in PATHS.items()}
    if a.trace:
        key = tuple(a.trace.split(":"))
        calls = {key: calls[key]}
    events = {}
    for key, fn in calls.items():   # warm-up of every shape
        events[key] = int(fn()["frame_bounds"][-1])
    ctx.synchronize()
    if a.trace:
        for _ in range(a.reps):
            calls[key]()
        ctx.synchronize()
        print(json.dumps({"bench": "events_sensor", "trace": a.trace, "trace_reps": a.reps, "frames": n, "events": events[key]}))
        ctx.close()
        return
    ms = {key: [] for key in calls}
    for _ in range(a.reps):
        for key, fn in calls.items():
            t_ms, out = timed(fn)
            ms[key].append(t_ms)
            del out
    for m in ("frame", "linear"):
        entry = {k: dict(spread(ms[(m, k)]), events=events[(m, k)]) for k in PATHS}
        for k in PATHS:
            entry[k]["over_plain"] = round(entry[k]["median_ms"] / entry["plain"]["median_ms"], 3)
        line["modes"][m] = entry

    if a.parent_lib:
        _lib.load()   # (the HIP runtime both libraries link against is in the process)
        libs = {"new": ctx._lib, "parent": C.CDLL(os.path.abspath(a.parent_lib))}
        for name in ("nsof_create", "nsof_destroy", "nsof_set_stream", "nsof_synchronize", "nsof_events_from_frames_count_dev",
                     "nsof_events_from_frames_emit_dev", "nsof_events_from_frames_sensor_count_dev",
                     "nsof_events_from_frames_sensor_emit_dev"):
            fn = getattr(libs["parent"], name)
            fn.restype, fn.argtypes = _lib.SIGNATURES[name]
        ptrs = {}
        for which in ("parent", "new"):   # a fresh context of each library: the one above has the workspace of the paths it ran
            ptrs[which] = C.c_void_p()
            assert libs[which].nsof_create(0, C.byref(ptrs[which])) == 0
            assert libs[which].nsof_set_stream(ptrs[which], C.c_void_p(stream.cuda_stream)) == 0
        lut = nsof.linear_response()
        c = units(THRESHOLD)
        q = rate_q(NOISE["rate_hz"])
        st = C.byref(_lib.EventsSensor(REFRACTORY_US, NOISE["seed"], 0, q, q, None, None))
        common = (frames.data_ptr(), frames.stride(1), frames.stride(0), n, H, W, times.ctypes.data, lut.ctypes.data, c, c, None, None,
                  _lib.EVENTS_REF_FIRST)
        stamp = {"frame": _lib.EVENTS_T_FRAME, "linear": _lib.EVENTS_T_LINEAR}
        # the bounds of each stream, from the new library (the parent's must come out equal: its emit pass writes nothing otherwise)
        bounds = {k: np.empty(n + 1, np.int64) for k in ("plain", "sensor_frame", "sensor_linear")}
        assert libs["new"].nsof_events_from_frames_count_dev(ptrs["new"], *common, bounds["plain"].ctypes.data) == 0
        for m in stamp:
            assert libs["new"].nsof_events_from_frames_sensor_count_dev(ptrs["new"], *common, stamp[m], st,
                                                                        bounds["sensor_" + m].ctypes.data) == 0
        totals = {k: int(b[n]) for k, b in bounds.items()}
        cap = max(totals.values())
        x, y = (torch.empty(cap, dtype=torch.int16, device=dev) for _ in range(2))
        p = torch.empty(cap, dtype=torch.int8, device=dev)
        t = torch.empty(cap, dtype=torch.int64, device=dev)
        ref = torch.empty((H, W), dtype=torch.int32, device=dev)
        t_ok = torch.empty((H, W), dtype=torch.int64, device=dev)
        outs = (x.data_ptr(), y.data_ptr(), p.data_ptr(), t.data_ptr(), ref.data_ptr())

        # what -> (the entry's name, its arguments after the common ones, the stream it writes or None)
        whats = {"count": ("nsof_events_from_frames_count_dev", (bounds["plain"].ctypes.data,), None)}
        for m in stamp:
            whats["emit_" + m] = ("nsof_events_from_frames_emit_dev", (bounds["plain"].ctypes.data, stamp[m], 1, -1, totals["plain"]) + outs,
                                  "plain")
        for m in stamp:   # refractory time and noise together, the "both" of the paths above
            b = bounds["sensor_" + m].ctypes.data
            whats["sensor_count_" + m] = ("nsof_events_from_frames_sensor_count_dev", (stamp[m], st, b), None)
            whats["sensor_emit_" + m] = ("nsof_events_from_frames_sensor_emit_dev",
                                         (b, stamp[m], 1, -1, totals["sensor_" + m]) + outs + (st, t_ok.data_ptr()), "sensor_" + m)

        def entry_call(which, what):
            name, args, _ = whats[what]
            rc = getattr(libs[which], name)(ptrs[which], *common, *args)
            assert rc == 0, (which, what, rc)

        sums = {}
        for which in ("parent", "new"):   # warm-up, and the two libraries' streams compared after every emit entry
            sums[which] = {}
            for what, (_, _, written) in whats.items():
                for v in (x, y, p, t, ref, t_ok):
                    v.zero_()
                torch.cuda.synchronize(dev)
                entry_call(which, what)
                torch.cuda.synchronize(dev)
                if written:
                    sums[which][what] = [int(v[:totals[written]].to(torch.int64).sum()) for v in (x, y, p, t)] + \
                                        [int(ref.to(torch.int64).sum()), int(t_ok.sum())]
        pm = {(which, what): [] for which in libs for what in whats}
        for r in range(a.reps):
            for what in whats:
                # who goes first changes every round: the second call of a pair took about half a percent longer, whichever
                # library it was (the same library loaded twice showed it)
                for which in (("parent", "new"), ("new", "parent"))[r % 2]:
                    pm[(which, what)].append(timed(lambda: entry_call(which, what))[0])
        check = {"same_stream_sums": sums["new"] == sums["parent"], "events": totals}
        for what in whats:
            new, par = spread(pm[("new", what)]), spread(pm[("parent", what)])
            check[what] = {"new": new, "parent": par, "within_parent_range": new["median_ms"] <= par["max_ms"]}
        line["vs_parent"] = check
        for which in ptrs:
            libs[which].nsof_destroy(ptrs[which])
    line["not_measured"] = ["hardware counters", "frame sizes other than 1080p", "rate planes (hot pixels)", "chunked runs",
                            "a given t_ok plane"]
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
