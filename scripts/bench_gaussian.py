"""The Gaussian window (flags = 256: k_update_matrices + k_gauss_blur_solve per iteration) against the box window, on 256
device-resident pairs of 1920x1080, parameter set A, in one process.

Legs (each timed on its own after warm-up, then once more with the library's kernel scopes on):
  box15     flags 0,   winsize 15: the fused exact iteration (k_iterate_x)
  gauss15   flags 256, winsize 15: the new route
  box33     flags 0,   winsize 33: the unfused exact pair (k_update_matrices + k_blur_colsum + k_blur_rowsolve)
  gauss33   flags 256, winsize 33: the new route at the widest window of its LDS kernel
plus the new kernel alone at full resolution (nsof_stage_gauss_blur_solve on `--stage-pairs` pairs of matrices, 20 B/px:
far more than the 256 MiB Infinity Cache holds), windows 15 and 33.

Per leg: pairs/s, and per scope (blur_solve, update_matrices, iterate) the time per launch.  For the new kernel: the bytes
its algorithm needs -- 28 B/px: 20 read (5 planes of M), 8 written (the flow) -- over its time, as a share of 8 TB/s.  In a
whole call a scope's launches cover every pyramid level, so its bytes are summed over the levels.

    python scripts/bench_gaussian.py [--pairs 256] [--steps 5] [--warmup 2] [--stage-pairs 64]
                                     [--out profiles/gaussian_window_bench.json]
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

H, W = 1080, 1920
HBM_BYTES_PER_S = 8e12
GAUSS_BYTES_PER_PX = 28


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


def _scopes(ctx, lib, kernels, fn, steps):
    """-> {scope name: {"ms_per_step", "launches_per_step", "ms_per_launch"}} over `steps` runs of fn."""
    ctx.prof_enable(*kernels)
    for k in kernels:
        ctx.prof_collect(k)
    for _ in range(steps):
        fn()
    ctx.synchronize()
    out = {}
    for k in kernels:
        ms, n = ctx.prof_collect(k)
        if n:
            out[lib.nsof_kernel_name(k).decode()] = {"ms_per_step": round(ms / steps, 4), "launches_per_step": n // steps,
                                                     "ms_per_launch": round(ms / n, 4)}
    ctx.prof_enable()
    return out


def _share(px, ms):
    """Share of the HBM peak of a Gaussian blur-and-solve over px pixels in ms."""
    return round(GAUSS_BYTES_PER_PX * px / (ms * 1e-3) / HBM_BYTES_PER_S, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stage-pairs", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    g.build_native()
    import nsof
    from nsof import _lib, synth
    from nsof.farneback import PARAMS_A, FarnebackParams, farneback_batch
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    ctx = nsof.Context(0)
    n = args.pairs
    base = [synth.make_pair(s, H, W) for s in range(4)]
    prev = torch.from_numpy(np.stack([base[i % 4][0] for i in range(n)])).to(dev)
    nxt = torch.from_numpy(np.stack([base[i % 4][1] for i in range(n)])).to(dev)
    flow = torch.empty((n, H, W, 2), dtype=torch.float32, device=dev)
    kernels = [_lib.K_ITERATE, _lib.K_UPDMAT, _lib.K_BLUR]
    a = PARAMS_A
    levels = nsof.effective_levels(W, H, a.pyr_scale, a.levels)
    level_px = sum(np.prod(nsof.level_size(W, H, a.pyr_scale, k)[:2], dtype=np.int64) for k in range(levels + 1))
    res = {"metric": "gaussian_window_bench", "device": torch.cuda.get_device_name(0), "pairs": n, "shape": [H, W],
           "params": "A (pyr_scale 0.5, levels 3, iterations 3, poly_n 5, poly_sigma 1.2), winsize and flags per leg",
           "steps": args.steps, "gauss_bytes_per_px": GAUSS_BYTES_PER_PX, "hbm_peak_bytes_per_s": HBM_BYTES_PER_S, "legs": {}}
    for name, winsize, flags in (("box15", 15, 0), ("gauss15", 15, 256), ("box33", 33, 0), ("gauss33", 33, 256)):
        p = FarnebackParams(a.pyr_scale, a.levels, winsize, a.iterations, a.poly_n, a.poly_sigma, flags)

        def step(p=p):
            farneback_batch(prev, nxt, flow, n, H, W, p, ctx=ctx)
        med, mn = _timed(step, args.steps, args.warmup, ctx.synchronize)
        leg = {"winsize": winsize, "flags": flags, "step_ms_median": round(med * 1e3, 3), "step_ms_min": round(mn * 1e3, 3),
               "pairs_per_s": round(n / med, 1), "scopes": _scopes(ctx, lib, kernels, step, args.steps)}
        if flags:
            # one launch per level and iteration: the scope's time per step covers iterations * (all levels) * pairs pixels
            leg["blur_solve_share_of_hbm_peak_all_levels"] = _share(a.iterations * int(level_px) * n,
                                                                    leg["scopes"]["blur_solve"]["ms_per_step"])
        res["legs"][name] = leg
    del prev, nxt, flow

    # the new kernel alone, full resolution
    sp = args.stage_pairs
    M = torch.rand((sp, 5, H, W), dtype=torch.float32, device=dev)
    out = torch.empty((sp, H, W, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    res["stage_1080p"] = {"pairs": sp}
    for winsize in (15, 33):
        def stage(winsize=winsize):
            ctx.check(lib.nsof_stage_gauss_blur_solve(ctx.ptr, sp, M.data_ptr(), W, H, winsize, out.data_ptr()), "stage")
        _timed(stage, 1, args.warmup, ctx.synchronize)
        sc = _scopes(ctx, lib, [_lib.K_BLUR], stage, max(args.steps, 10))["blur_solve"]
        res["stage_1080p"][f"winsize{winsize}"] = {"ms_per_launch": sc["ms_per_launch"],
                                                   "share_of_hbm_peak": _share(sp * H * W, sc["ms_per_launch"])}
    ctx.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
