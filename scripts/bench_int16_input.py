"""16-bit frames on the device (the typed entries nsof_farneback_px*) against 8-bit and float32 frames, in one process.

Legs (each path timed on its own after warm-up; flows compared for identity where the pixel values are the same):
  batch    256 device-resident 1080p pairs, parameter set A: u8, u16, s16 and f32 frames holding the same values
           (pairs/s, per-kernel ms and launches per step)
  lists    device crop lists 64 x 520x200 and 8 x 1600x900 (set A): u16 against u8 (farneback_pairs_16_dev /
           farneback_pairs_dev)
  lone     a lone 1080p uint16 call, host to host, through calcOpticalFlowFarneback
  config4  the five datasets' calls as uint16 host lists (values x257): nsof_farneback_px_batch (the frames cross PCIe at
           2 B/px) against farneback_pairs' float32 staging

    python scripts/bench_int16_input.py [--pairs 256] [--steps 5] [--warmup 2] [--legs batch,lists,lone,config4]
                                        [--out profiles/int16_input_bench.json]
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


def _timed(fn, steps, warmup, sync):
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


def _profiled(ctx, lib, kernels, fn, steps):
    ctx.prof_enable(*kernels)
    for _ in range(steps):
        fn()
    ctx.synchronize()
    prof = {lib.nsof_kernel_name(k).decode(): ctx.prof_collect(k) for k in kernels}
    ctx.prof_enable()
    return ({n: round(ms / steps, 3) for n, (ms, _) in prof.items()}, {n: c // steps for n, (_, c) in prof.items()})


def leg_batch(nsof, torch, dev, n, steps, warmup):
    from nsof import _lib, synth
    from nsof.farneback import PARAMS_A as P, farneback_batch
    H, W = 1080, 1920   # noqa: N806
    ctx = nsof.Context(0)
    lib = _lib.load()
    base = [synth.make_pair(s, H, W) for s in range(4)]
    prev = np.stack([base[i % 4][0] for i in range(n)])
    nxt = np.stack([base[i % 4][1] for i in range(n)])
    frames = {k: (torch.from_numpy(prev.astype(k)).to(dev), torch.from_numpy(nxt.astype(k)).to(dev))
              for k in ("uint8", "uint16", "int16", "float32")}
    flows = {k: torch.empty((n, H, W, 2), dtype=torch.float32, device=dev) for k in frames}
    kernels = [_lib.K_PREP, _lib.K_POLYEXP, _lib.K_UPSAMPLE, _lib.K_ITERATE, _lib.K_UPDMAT, _lib.K_BLUR]
    out = {"pairs": n, "shape": [H, W], "params": "A"}
    for k in frames:
        def step(k=k):
            farneback_batch(frames[k][0], frames[k][1], flows[k], n, H, W, P, ctx=ctx)
        med, mn = _timed(step, steps, warmup, ctx.synchronize)
        kms, launches = _profiled(ctx, lib, kernels, step, steps)
        out[k] = {"step_ms_median": round(med * 1e3, 3), "step_ms_min": round(mn * 1e3, 3), "pairs_per_s": round(n / med, 1),
                  "kernel_ms_per_step": kms, "launches_per_step": launches}
    out["flow_identical"] = all(bool(torch.equal(flows["uint8"], flows[k])) for k in flows)
    for k in ("uint16", "int16", "float32"):
        out[f"{k}_over_uint8_pairs_per_s"] = round(out[k]["pairs_per_s"] / out["uint8"]["pairs_per_s"], 4)
    ctx.close()
    return out


def leg_lists(nsof, torch, dev, steps, warmup):
    from nsof import _lib, synth
    from nsof.farneback import PARAMS_A as P, farneback_pairs_16_dev, farneback_pairs_dev
    ctx = nsof.Context(0)
    lib = _lib.load()
    kernels = [_lib.K_PREP, _lib.K_POLYEXP, _lib.K_ITERATE]
    out = {}
    for label, n, h, w, fh, fw in (("64x520x200", 64, 200, 520, 480, 1100), ("8x1600x900", 8, 900, 1600, 1000, 1700)):
        a, b = synth.make_pair(7, fh, fw)
        frames = {"uint8": (torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)),
                  "uint16": (torch.from_numpy(a.astype(np.uint16)).to(dev), torch.from_numpy(b.astype(np.uint16)).to(dev))}
        crops = [((7 * i) % (fh - h), (13 * i + (i & 1)) % (fw - w)) for i in range(n)]
        res = {}
        flows = {k: torch.empty((n, h, w, 2), dtype=torch.float32, device=dev) for k in frames}
        for k, fn in (("uint8", farneback_pairs_dev), ("uint16", farneback_pairs_16_dev)):
            ta, tb = frames[k]
            pairs = [(ta[y:y + h, x:x + w], tb[y:y + h, x:x + w]) for (y, x) in crops]

            def step(fn=fn, pairs=pairs, k=k):
                fn(pairs, list(flows[k]), P, ctx=ctx)
            med, mn = _timed(step, steps, warmup, ctx.synchronize)
            kms, launches = _profiled(ctx, lib, kernels, step, steps)
            res[k] = {"ms_median": round(med * 1e3, 3), "ms_min": round(mn * 1e3, 3), "kernel_ms_per_list": kms,
                      "launches_per_list": launches}
        res["flow_identical"] = bool(torch.equal(flows["uint8"], flows["uint16"]))
        res["uint16_over_uint8_time"] = round(res["uint16"]["ms_median"] / res["uint8"]["ms_median"], 4)
        out[label] = res
    ctx.close()
    return out


def leg_lone(nsof, steps):
    from nsof import synth
    from nsof.farneback import PARAMS_A as P
    ctx = nsof.Context(0)
    a, b = (x.astype(np.uint16) * 257 for x in synth.make_pair(0, 1080, 1920))
    med, mn = _timed(lambda: nsof.calcOpticalFlowFarneback(a, b, None, **P.as_kwargs(), ctx=ctx), steps, 3, lambda: None)
    f16 = nsof.calcOpticalFlowFarneback(a, b, None, **P.as_kwargs(), ctx=ctx)
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    med32, mn32 = _timed(lambda: nsof.calcOpticalFlowFarneback(fa, fb, None, **P.as_kwargs(), ctx=ctx), steps, 3,
                         lambda: None)
    f32 = nsof.calcOpticalFlowFarneback(fa, fb, None, **P.as_kwargs(), ctx=ctx)
    ctx.close()
    return {"uint16_ms_median": round(med * 1e3, 3), "uint16_ms_min": round(mn * 1e3, 3),
            "float32_ms_median": round(med32 * 1e3, 3), "float32_ms_min": round(mn32 * 1e3, 3), "n": steps,
            "flow_identical_to_float32": bool(np.array_equal(f16.view(np.int32), f32.view(np.int32)))}


def leg_config4(nsof, steps):
    from nsof import _lib
    from nsof import workload as wl
    from nsof.farneback import farneback_pairs
    with np.load(os.path.join(ROOT, "tests", "golden", "gating_stacks.npz")) as z:
        stacks = {k: z[k] for k in z.files}
    calls, _ = wl.mixed_workload(stacks)
    mpx = sum(c.prev.size for c in calls) / 1e6
    groups = {}
    for c in calls:   # one host list per parameter set, as farneback_pairs' callers pass them
        groups.setdefault(c.params, []).append((c.prev.astype(np.uint16) * 257, c.next.astype(np.uint16) * 257))
    ctx = nsof.Context(0)
    native = {p: [np.empty((a.shape[0], a.shape[1], 2), np.float32) for a, _ in g] for p, g in groups.items()}
    staged = {p: [np.empty_like(f) for f in fl] for p, fl in native.items()}

    def run_native():
        for p, g in groups.items():
            descs = (_lib.PairDesc * len(g))()
            for d, (a, b), f in zip(descs, g, native[p]):
                d.prev, d.prev_stride, d.next, d.next_stride = a.ctypes.data, a.strides[0], b.ctypes.data, b.strides[0]
                d.width, d.height, d.flow, d.flow_stride = a.shape[1], a.shape[0], f.ctypes.data, f.strides[0]
            kw = p.as_kwargs()
            ctx.check(ctx._lib.nsof_farneback_px_batch(ctx.ptr, _lib.PIXEL_U16, len(g), descs, *(kw[k] for k in (
                "pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags"))), "px_batch")

    def run_staged():
        for p, g in groups.items():
            farneback_pairs(g, p, staged[p], ctx=ctx)
    out = {"workload": "config 4 calls as uint16 host lists (values x257), one list per parameter set",
           "calls": len(calls), "lists": len(groups), "megapixels": round(mpx, 1)}
    for k, fn in (("native_px_batch", run_native), ("float32_staging", run_staged)):
        med, mn = _timed(fn, steps, 1, lambda: None)
        out[k] = {"s_median": round(med, 4), "s_min": round(mn, 4), "calls_per_s": round(len(calls) / med, 1)}
    out["flow_identical"] = all(np.array_equal(a, b) for p in native for a, b in zip(native[p], staged[p]))
    out["native_speedup"] = round(out["float32_staging"]["s_median"] / out["native_px_batch"]["s_median"], 3)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="batch,lists,lone,config4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    g.build_native()
    import nsof
    dev = torch.device("cuda", 0)
    legs = args.legs.split(",")
    res = {"metric": "int16_input_bench", "steps": args.steps, "device": torch.cuda.get_device_name(0)}
    if "batch" in legs:
        res["batch_1080p"] = leg_batch(nsof, torch, dev, args.pairs, args.steps, args.warmup)
    if "lists" in legs:
        res["device_lists"] = leg_lists(nsof, torch, dev, args.steps, args.warmup)
    if "lone" in legs:
        res["lone_1080p_uint16_host_to_host"] = leg_lone(nsof, max(10, args.steps))
    if "config4" in legs:
        res["config4_uint16_host_lists"] = leg_config4(nsof, max(3, args.steps // 2))
    same = all(v.get("flow_identical", True) if isinstance(v, dict) else True for v in res.values())
    same = same and all(r["flow_identical"] for r in res.get("device_lists", {}).values())
    same = same and res.get("lone_1080p_uint16_host_to_host", {}).get("flow_identical_to_float32", True)
    res["all_flows_identical"] = bool(same)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
