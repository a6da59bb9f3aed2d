"""Float work lists against 8-bit work lists, each leg u8 against f32 in one process:

  (a) the config-3 sparse stream (1280x720, 5 k background events, silent 0.5 V) through pipeline.events_to_roi_flows
      with surface_dtype "uint8" against "float32": the flow stage time (the ROI crops of every pair as one list);
  (b) 64 device-resident crops of 520x200 of 1080p frames as one list (farneback_pairs_dev / farneback_pairs_f32_dev),
      at crop positions that are not a constant step apart, so the list runs on the work-list kernels and not on the
      uniform driver (which takes equal shapes at constant strides); per-kernel times from nsof_prof_enable;
  (d) the same for 8 crops of 1600x900 (a fourth pyramid level at pyr_scale 0.5: 19 taps, decimation by 8);
  (c) the five datasets' gated and full-frame calls as one host list per parameter set (scripts/bench_config4.py's
      workload, workload.run_calls) on uint8 frames, their float32 copies and uint16 copies (x257); the uint16 leg
      includes the host conversion, timed on its own as well.

Prints one JSON line (and writes it to --out).

    python scripts/bench_float_worklists.py [--steps 10] [--out profiles/float_worklists_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]

import numpy as np  # noqa: E402


def _median_time(fn, steps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        sync()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times)


def leg_config3(nsof, steps):
    from nsof import gating, pipeline, synth
    from nsof.farneback import PARAMS_A
    H, W, every = 720, 1280, 33   # noqa: N806
    cfg = gating.GatingConfig(MEMSIZE=20, EXTEND_HEIGHT_UPPER=20, EXTEND_HEIGHT_LOWER=20, EXTEND_WIDTH_LEFT=20,
                              EXTEND_WIDTH_RIGHT=20, THRES=240, FLAG=1, farneback_params=PARAMS_A, bug_compatible=False)
    x, y, p, t = synth.make_events(2024, W, H, n_background=5_000)
    out = {"workload": "config-3 sparse stream 1280x720, 5 k background events, silent 0.5 V, FLAG 1, params A"}
    with nsof.Context(0) as c:
        rects_of = {}
        for dt in ("uint8", "float32"):
            flow_s, calls = [], None
            for i in range(steps + 1):   # the first run warms up
                tm = {}
                _, rects, _ = pipeline.events_to_roi_flows(x, y, p, t, (H, W), cfg, slice_us=1000, active_v=-6.0, silent_v=0.5,
                                                           snapshot_every=every, ctx=c, timings=tm, max_rects=256,
                                                           surface_dtype=dt)
                if i:
                    flow_s.append(tm["flow_s"])
                calls, pixels, frames = tm["roi_calls"], tm["roi_pixels"], tm["frames"]
            rects_of[dt] = rects
            med = statistics.median(flow_s)
            out[dt] = {"roi_calls": calls, "roi_pixels": pixels, "frames": frames, "flow_ms_median": round(med * 1e3, 3),
                       "flow_ms_min": round(min(flow_s) * 1e3, 3), "pairs_per_s": round((frames - 1) / med, 1),
                       "roi_calls_per_s": round(calls / med, 1)}
    out["rects_identical"] = rects_of["uint8"] == rects_of["float32"]
    out["f32_over_u8"] = round(out["float32"]["pairs_per_s"] / out["uint8"]["pairs_per_s"], 4)
    return out


def leg_device_crops(nsof, torch, steps, n=64, ch=200, cw=520):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    frames = {"u8": torch.randint(0, 256, (2, 1080, 1920), dtype=torch.uint8, device=dev, generator=g)}
    frames["f32"] = frames["u8"].float()
    canvas = torch.zeros((n, ch, cw, 2), dtype=torch.float32, device=dev)
    flows = [canvas[i] for i in range(n)]
    p = nsof.farneback.PARAMS_A
    from nsof import _lib
    # crop origins quadratic in i: no constant pointer step between items (a constant step with equal shapes and dense
    # consecutive flows is what nsof_farneback_list_core hands to the uniform driver)
    origins = [((7 * i * i + 3 * i) % (1080 - ch), (37 * i + (i * i) % 11) % (1920 - cw)) for i in range(n)]
    steps_x = {origins[i + 1][1] - origins[i][1] for i in range(n - 1)}
    steps_y = {origins[i + 1][0] - origins[i][0] for i in range(n - 1)}
    assert len(steps_x) > 1 or len(steps_y) > 1
    out = {"workload": f"{n} crops of {cw}x{ch} of 1080p frames in HBM at non-uniform positions, one work list, params A"}
    ctx = nsof.Context(0)
    kernels = [_lib.K_PREP, _lib.K_POLYEXP, _lib.K_UPSAMPLE, _lib.K_ITERATE]
    results = {}
    for k, fn in (("u8", nsof.farneback_pairs_dev), ("f32", nsof.farneback_pairs_f32_dev)):
        fr = frames[k]
        pairs = [(fr[0, y:y + ch, x:x + cw], fr[1, y:y + ch, x:x + cw]) for (y, x) in origins]
        med, mn = _median_time(lambda: fn(pairs, flows, p, ctx=ctx), steps, 3, ctx.synchronize)
        results[k] = canvas.clone()
        ctx.prof_enable(*kernels)
        for _ in range(steps):
            fn(pairs, flows, p, ctx=ctx)
        ctx.synchronize()
        prof = {_lib.load().nsof_kernel_name(kid).decode(): ctx.prof_collect(kid) for kid in kernels}
        ctx.prof_enable()
        out[k] = {"ms_per_list_median": round(med * 1e3, 3), "ms_per_list_min": round(mn * 1e3, 3),
                  "pairs_per_s": round(n / med, 1),
                  "kernel_ms_per_list": {name: round(ms / steps, 4) for name, (ms, _) in prof.items()},
                  "launches_per_list": {name: cnt // steps for name, (_, cnt) in prof.items()}}
    out["flow_identical"] = bool(torch.equal(results["u8"], results["f32"]))
    out["f32_over_u8"] = round(out["f32"]["pairs_per_s"] / out["u8"]["pairs_per_s"], 4)
    ctx.close()
    return out


def leg_config4(nsof, steps):
    from nsof import workload as wl
    with np.load(os.path.join(ROOT, "tests", "golden", "gating_stacks.npz")) as z:
        stacks = {k: z[k] for k in z.files}
    calls, _ = wl.mixed_workload(stacks)
    n = len(calls)
    mpx = sum(c.prev.size for c in calls) / 1e6
    out = {"workload": "config 4: grasp+autodriving+uav+uavnew2+tabletennis, gated ROI + full-frame calls as host lists",
           "calls": n, "megapixels": round(mpx, 1)}
    ctx = nsof.Context(0)
    u8 = [(c.prev, c.next) for c in calls]

    def with_frames(frames):
        out_calls = []
        for c, (a, b) in zip(calls, frames):
            out_calls.append(wl.FlowCall(c.dataset, c.pair, c.kind, c.rect, c.params, a, b, c.flow, c.paste_to))
        return out_calls

    ref = None
    for k in ("uint8", "float32", "uint16"):
        if k == "uint8":
            cs = calls
        elif k == "float32":   # float32 copies made once, outside the timing
            cs = with_frames([(a.astype(np.float32), b.astype(np.float32)) for a, b in u8])
        else:                  # uint16 copies (x257): converted to float32 inside every timed call
            cs = with_frames([(a.astype(np.uint16) * 257, b.astype(np.uint16) * 257) for a, b in u8])
        med, mn = _median_time(lambda: wl.run_calls(cs, ctx=ctx), steps, 1, ctx.synchronize)
        flows = [c.flow.copy() for c in cs]
        if k == "uint16":
            flows = None   # other values, other flow
        elif ref is None:
            ref = flows
        else:
            out["float32_flow_identical_to_uint8"] = bool(all(np.array_equal(a, b) for a, b in zip(ref, flows)))
        out[k] = {"s_median": round(med, 4), "s_min": round(mn, 4), "calls_per_s": round(n / med, 1),
                  "mpx_per_s": round(mpx / med, 1)}
    # the host share of the uint16 leg: the conversion to float32 (what farneback_pairs does before the native call)
    frames16 = [(a.astype(np.uint16) * 257, b.astype(np.uint16) * 257) for a, b in u8]
    from nsof.farneback import _f32_host_frames
    conv = []
    for _ in range(max(3, steps // 2)):
        t0 = time.perf_counter()
        with ctx.lock:
            _f32_host_frames(frames16, ctx)
        conv.append(time.perf_counter() - t0)
    out["uint16_host_conversion_s_median"] = round(statistics.median(conv), 4)
    out["float32_over_uint8"] = round(out["float32"]["calls_per_s"] / out["uint8"]["calls_per_s"], 4)
    out["uint16_over_uint8"] = round(out["uint16"]["calls_per_s"] / out["uint8"]["calls_per_s"], 4)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--legs", default="a,b,c,d")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    g.build_native()
    import nsof
    res = {"metric": "float_worklists_bench", "device": torch.cuda.get_device_name(0), "steps": args.steps}
    legs = args.legs.split(",")
    if "a" in legs:
        res["a_config3_sparse"] = leg_config3(nsof, args.steps)
    if "b" in legs:
        res["b_device_crops_520x200_x64"] = leg_device_crops(nsof, torch, args.steps)
    if "d" in legs:   # large crops: a fourth level at pyr_scale 0.5 (19 taps, decimation by 8)
        res["d_device_crops_1600x900_x8"] = leg_device_crops(nsof, torch, args.steps, n=8, ch=900, cw=1600)
    if "c" in legs:
        res["c_config4_host_lists"] = leg_config4(nsof, max(3, args.steps // 3))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
