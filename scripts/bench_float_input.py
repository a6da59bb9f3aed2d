"""Float32 frames against 8-bit frames: 256 device-resident 1080p pairs, parameter set A, through
nsof_farneback_f32_batch_dev and nsof_farneback_u8_batch_dev in the same process (same pixel values, so the same flow).

Prints one JSON line: pairs/s of each path and their ratio, per-kernel times per step (nsof_prof_enable), the f32
pyramid stage's achieved bandwidth on its algorithmic bytes (4 B/px read of the full-resolution frame per level + the
f32 level image written), and the lone-call 1080p f32 host-to-host time.

    python scripts/bench_float_input.py [--pairs 256] [--steps 5] [--warmup 2] [--out profiles/float_input_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lone", type=int, default=20, help="timed lone host-to-host calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    g.build_native()
    import nsof
    from nsof import _lib, synth
    from nsof.farneback import PARAMS_A as P, farneback_batch

    H, W, n = 1080, 1920, args.pairs
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    base = [synth.make_pair(s, H, W) for s in range(4)]
    prev_u8 = torch.from_numpy(np.stack([base[i % 4][0] for i in range(n)])).to(dev)
    next_u8 = torch.from_numpy(np.stack([base[i % 4][1] for i in range(n)])).to(dev)
    prev_f32, next_f32 = prev_u8.float(), next_u8.float()
    flows = {k: torch.empty((n, H, W, 2), dtype=torch.float32, device=dev) for k in ("u8", "f32")}
    frames = {"u8": (prev_u8, next_u8), "f32": (prev_f32, next_f32)}
    kernels = [_lib.K_PREP, _lib.K_POLYEXP, _lib.K_UPSAMPLE, _lib.K_ITERATE, _lib.K_UPDMAT, _lib.K_BLUR]

    def step(k):
        farneback_batch(frames[k][0], frames[k][1], flows[k], n, H, W, P, ctx=ctx)

    res = {"metric": "float_input_bench", "pairs": n, "shape": [H, W], "params": "A", "steps": args.steps,
           "device": torch.cuda.get_device_name(0)}
    for k in ("u8", "f32"):   # interleaved order would mix the profiles; each path is timed on its own after warm-up
        for _ in range(args.warmup):
            step(k)
        ctx.synchronize()
        times = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            step(k)
            ctx.synchronize()
            times.append(time.perf_counter() - t0)
        med = statistics.median(times)
        ctx.prof_enable(*kernels)
        for _ in range(args.steps):
            step(k)
        ctx.synchronize()
        prof = {nsof_name: ctx.prof_collect(kid) for kid, nsof_name in
                ((kid, _lib.load().nsof_kernel_name(kid).decode()) for kid in kernels)}
        ctx.prof_enable()
        res[k] = {"step_ms_median": round(med * 1e3, 3), "step_ms_min": round(min(times) * 1e3, 3),
                  "pairs_per_s": round(n / med, 1),
                  "kernel_ms_per_step": {name: round(ms / args.steps, 3) for name, (ms, _) in prof.items()},
                  "launches_per_step": {name: cnt // args.steps for name, (_, cnt) in prof.items()}}
    same = bool(torch.equal(flows["u8"], flows["f32"]))
    res["flow_identical"] = same
    res["f32_over_u8_pairs_per_s"] = round(res["f32"]["pairs_per_s"] / res["u8"]["pairs_per_s"], 4)

    # algorithmic bytes of the f32 pyramid stage per step: every level reads both full-resolution f32 frames of a pair
    # once and writes its f32 level images
    L = nsof.effective_levels(W, H, P.pyr_scale, P.levels)
    prep_bytes = 0
    for lv in range(L + 1):
        wk, hk, _, _ = nsof.level_size(W, H, P.pyr_scale, lv)
        prep_bytes += 2 * n * (4 * W * H + 4 * wk * hk)
    prep_name = _lib.load().nsof_kernel_name(_lib.K_PREP).decode()
    prep_ms = res["f32"]["kernel_ms_per_step"][prep_name]
    res["f32_pyramid"] = {"algorithmic_bytes_per_step": prep_bytes, "ms_per_step": prep_ms,
                          "achieved_GBps": round(prep_bytes / (prep_ms * 1e-3) / 1e9, 1) if prep_ms else None}

    a, b = (x.astype(np.float32) for x in base[0])
    for _ in range(3):
        nsof.calcOpticalFlowFarneback(a, b, None, **P.as_kwargs(), ctx=ctx)
    lone = []
    for _ in range(args.lone):
        t0 = time.perf_counter()
        nsof.calcOpticalFlowFarneback(a, b, None, **P.as_kwargs(), ctx=ctx)
        lone.append(time.perf_counter() - t0)
    res["lone_1080p_f32_host_to_host_ms"] = {"median": round(statistics.median(lone) * 1e3, 3),
                                             "min": round(min(lone) * 1e3, 3), "n": args.lone}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
