#!/usr/bin/env python3
"""Event streams from frame sequences (``nsof.events_from_frames_dev``); prints one JSON line.

    python scripts/bench_events_from_frames.py [--frames 64 --reps 10 --host-frames 64 --out profiles/events_from_frames.json]

Input: --frames frames of 1080p drifting texture (``synth.make_sequence(7, n, pad=192)``: consecutive ``make_pair`` shifts of
one texture, 2.5 / -1.25 px and 0.2 degrees per frame), 33333 us apart, threshold 10 grey levels, ``ref="first"`` (a camera
that has settled on the first frame: with ``ref=None`` the first frame alone gives a burst of a dozen events per pixel).

  device   per timestamp mode, after a warm-up, --reps rounds that alternate the three library calls, each between two
           device events on the context's stream:
             count         ``nsof_events_from_frames_count_dev`` (count pass, two scans, the copy of the bounds, synchronise)
             emit frame    ``nsof_events_from_frames_emit_dev`` with frame time stamps: the count pass again, then the emit pass
             emit linear   the same with linear time stamps: count, emit into the workspace, radix sort, unpack
           median and min-max of each in ms, and from the medians ``emit_pass_ms`` = emit frame - count and ``reorder_ms`` =
           emit linear - emit frame (differences of whole calls, not kernel times: the count entry also copies the bounds
           and synchronises, and the linear emit pass writes 12 B per event where the frame one writes 13).  ``call`` is
           ``events_from_frames_dev`` as a user calls it (count + emit entries, output allocation): frames/s and events/s
           come from it.  Model bytes: every frame read twice (count, emit) plus 13 B per event written; linear adds the
           reorder's traffic -- 12 B per event written by the emit pass instead of 13, 8 B per event read by the sort's
           histogram, 24 B per event and radix pass (8 key bits each) and 12 + 13 B per event for the unpack.  The share of
           the 8 TB/s peak is those bytes over the call's median.  (The emit entry forms the counts again, so it reads the
           frames a third time; that read is not in the model.)
  host     the NumPy restatement of the model (tests/events_from_frames_ref.py) on the first --host-frames frames of the
           same input, host clock, once per mode; the device result is compared with it (x, y, p, t, frame_bounds, ref equal)
           and the device call on those frames is timed again (median of 5).
--trace runs the three library calls (count, emit frame, emit linear) --reps times after the warm-up and nothing else, for a
separate ``rocprofv3 --kernel-trace --stats`` run: every round then launches k_ef_count three times, k_ev_scan six times,
each k_ef_emit form, the sort's kernels and k_ef_unpack once.
Not measured: other frame sizes, the threshold plane, response tables other than the linear one, chunked runs."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd"), os.path.join(ROOT, "tests")]
HBM_PEAK = 8e12
H, W = 1080, 1920
FRAME_US = 33333
THRESHOLD = 10.0


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def model_bytes(n, events, linear, span_us):
    frames = 2 * n * H * W
    if not linear:
        return frames + 13 * events
    passes = (max(int(span_us).bit_length(), 1) + 7) // 8
    return frames + (12 + 8 + 24 * passes + 12 + 13) * events


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-frames", type=int, default=64)
    ap.add_argument("--trace", action="store_true", help="the three library calls --reps times and nothing else")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import _lib, synth
    from events_from_frames_ref import events_from_frames_ref, units
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    ctx.set_stream(stream.cuda_stream)
    n = a.frames
    frames_h = synth.make_sequence(7, n, H, W, pad=192)
    times = np.arange(n, dtype=np.int64) * FRAME_US
    frames = torch.from_numpy(frames_h).to(dev)
    lut = nsof.linear_response()
    c = units(THRESHOLD)
    line = {"bench": "events_from_frames", "frames": n, "frame_hw": [H, W], "frame_us": FRAME_US, "threshold_grey": THRESHOLD, "ref": "first",
            "reps": a.reps, "modes": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    bounds = np.empty(n + 1, np.int64)
    common = (frames.data_ptr(), frames.stride(1), frames.stride(0), n, H, W, times.ctypes.data, lut.ctypes.data, c, c, None, None,
              _lib.EVENTS_REF_FIRST, bounds.ctypes.data)

    def count():
        ctx.check(ctx._lib.nsof_events_from_frames_count_dev(ctx.ptr, *common), "count")

    count()
    total = int(bounds[n])
    x, y = (torch.empty(total, dtype=torch.int16, device=dev) for _ in range(2))
    p = torch.empty(total, dtype=torch.int8, device=dev)
    t = torch.empty(total, dtype=torch.int64, device=dev)
    ref = torch.empty((H, W), dtype=torch.int32, device=dev)

    def emit(mode):
        ctx.check(ctx._lib.nsof_events_from_frames_emit_dev(ctx.ptr, *common, mode, 1, -1, total, x.data_ptr(), y.data_ptr(), p.data_ptr(),
                                                            t.data_ptr(), ref.data_ptr()), "emit")

    calls = {"count": count, "emit_frame": lambda: emit(_lib.EVENTS_T_FRAME), "emit_linear": lambda: emit(_lib.EVENTS_T_LINEAR)}
    user = {m: (lambda m=m: nsof.events_from_frames_dev(frames, times, threshold=THRESHOLD, ref="first", timestamps=m, ctx=ctx)) for m in ("frame", "linear")}
    for fn in list(calls.values()) + list(user.values()):   # warm-up of every shape
        fn()
    ctx.synchronize()
    if a.trace:
        for _ in range(a.reps):
            for fn in calls.values():
                fn()
        ctx.synchronize()
        print(json.dumps({"bench": "events_from_frames", "trace_reps": a.reps, "frames": n, "events": total}))
        ctx.close()
        return
    ms = {k: [] for k in list(calls) + ["call_frame", "call_linear"]}
    for _ in range(a.reps):
        for k, fn in calls.items():
            ms[k].append(timed(fn)[0])
        for m, fn in user.items():
            t_ms, out = timed(fn)
            ms["call_" + m].append(t_ms)
            del out
    entry = {k: spread(v) for k, v in ms.items()}
    entry["emit_pass_ms"] = round(entry["emit_frame"]["median_ms"] - entry["count"]["median_ms"], 4)
    entry["reorder_ms"] = round(entry["emit_linear"]["median_ms"] - entry["emit_frame"]["median_ms"], 4)
    line["events"] = total
    line["device"] = entry
    span = int(times[-1] - times[0])
    for m in ("frame", "linear"):
        med = entry["call_" + m]["median_ms"] * 1e-3
        mb = model_bytes(n, total, m == "linear", span)
        line["modes"][m] = {"frames_per_s": round(n / med, 1), "events_per_s": round(total / med, 1), "model_bytes": mb,
                            "hbm_share": round(mb / med / HBM_PEAK, 4)}

    hn = min(a.host_frames, n)
    for m in ("frame", "linear"):
        t0 = time.perf_counter()
        want = events_from_frames_ref(frames_h[:hn], times[:hn], c, c, ref="first", timestamps=m)
        host_s = time.perf_counter() - t0
        got = nsof.events_from_frames_dev(frames[:hn], times[:hn], threshold=THRESHOLD, ref="first", timestamps=m, ctx=ctx)
        ctx.synchronize()
        same = bool(np.array_equal(got["frame_bounds"], want["frame_bounds"])) and \
            all(bool(np.array_equal(got[k].cpu().numpy(), want[k])) for k in ("x", "y", "p", "t", "ref"))
        del got
        dev_ms = statistics.median(timed(lambda: nsof.events_from_frames_dev(frames[:hn], times[:hn], threshold=THRESHOLD, ref="first",
                                                                             timestamps=m, ctx=ctx))[0] for _ in range(5))
        line["modes"][m]["host_numpy"] = {"frames": hn, "events": int(want["frame_bounds"][-1]), "host_s": round(host_s, 3),
                                          "device_ms_same_input": round(dev_ms, 3), "host_over_device": round(host_s * 1e3 / dev_ms, 1),
                                          "equal": same}
        del want
    line["not_measured"] = ["other frame sizes", "the threshold plane", "response tables other than the linear one", "chunked runs"]
    print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
