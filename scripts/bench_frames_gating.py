#!/usr/bin/env python3
"""Frame-driven gating in HBM against the host chain; prints one JSON line and writes it to --out.

    python scripts/bench_frames_gating.py [--frames 100 --reps 10 --out profiles/frames_gating_bench.json]

--frames seeded gray frames of 1080x1920 (a static texture, a bright box that moves, per-frame noise), m = n = 80
-> 13x24 grids, the script's 1000 Euler sub-steps per pair:
  compress:  ``frames.process_images_dev`` (two launches: the row pass over the 8-bit frames, the column pass over its
             float64 output), wall time per call over --reps calls ending in a synchronise, after a warm-up call; the
             bytes it must read (frames x 1080 x 1920) over that time, as a share of 8 TB/s
  array run: ``simulate_frames_dev`` (one launch, one thread per grid cell), the same way
  join:      ``pipeline.gating_stack_from_frames_dev`` from BGR frames (gray conversion, compress, array run)
  host:      ``frames.process_images`` (NumPy float64) + ``simulate_frames`` (the same launch with copies both ways) on the
             same frames, timed once; and whether the device results equal the host chain bit for bit"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]

HBM_PEAK = 8.0e12   # bytes/s


def make_frames(np, n, h, w):
    rng = np.random.default_rng(7)
    texture = rng.integers(30, 140, (h, w), dtype=np.uint8)
    out = np.empty((n, h, w), np.uint8)
    for f in range(n):
        fr = texture.copy()
        y, x = 100 + 6 * f, 80 + 14 * f
        fr[y:y + 240, x:x + 320] = 245
        fr[::7, ::5] += rng.integers(0, 8, fr[::7, ::5].shape, dtype=np.uint8)
        out[f] = fr
    return out


def timed(ctx, fn, reps):
    fn()                               # warm-up: code objects, buffers
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--cell", type=int, default=80)
    ap.add_argument("--sub-steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the host chain (and the equality check)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_gating_bench.json"))
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np
    import torch

    import nsof
    from nsof import frames, gating, pipeline
    dev = torch.device("cuda", 0)
    ctx = nsof.Context(0)
    n, h, w, cell = a.frames, a.height, a.width, a.cell
    host = make_frames(np, n, h, w)
    d_gray = torch.from_numpy(host).to(dev)
    d_bgr = d_gray.unsqueeze(-1).expand(n, h, w, 3).contiguous()   # equal channels: RGB2GRAY gives the gray frame back
    cfg = gating.GatingConfig(MEMSIZE=cell)
    torch.cuda.synchronize(dev)

    grids = frames.process_images_dev(d_gray, cell, cell, ctx=ctx)
    t_compress = timed(ctx, lambda: frames.process_images_dev(d_gray, cell, cell, out=grids, ctx=ctx), a.reps)
    t_array = timed(ctx, lambda: nsof.simulate_frames_dev(grids, n_sub_steps=a.sub_steps, ctx=ctx), max(1, a.reps // 3))
    t_join = timed(ctx, lambda: pipeline.gating_stack_from_frames_dev(d_bgr, cfg, n_sub_steps=a.sub_steps, ctx=ctx),
                   max(1, a.reps // 3))
    _, _, cur = nsof.simulate_frames_dev(grids, n_sub_steps=a.sub_steps, ctx=ctx)
    stack = pipeline.gating_stack_from_frames_dev(d_bgr, cfg, n_sub_steps=a.sub_steps, ctx=ctx)
    ctx.synchronize()
    read_bytes = n * h * w
    rec = {"workload": f"{n} gray frames {w}x{h}, m = n = {cell} -> {h // cell}x{w // cell} grids, {a.sub_steps} sub-steps per pair",
           "timing": "host clock around calls that end in a synchronise, after one warm-up call; no profiler attached",
           "compress_ms": round(t_compress * 1e3, 4), "compress_reps": a.reps,
           "compress_read_bytes": read_bytes, "compress_bytes_per_s": round(read_bytes / t_compress, 1),
           "compress_share_of_8TBps": round(read_bytes / t_compress / HBM_PEAK, 5),
           "array_run_ms": round(t_array * 1e3, 4), "join_ms": round(t_join * 1e3, 4),
           "join_equals_compress_plus_array_run": bool(torch.equal(stack, cur))}
    if not a.no_host:
        t0 = time.perf_counter()
        comp = frames.process_images(list(host), cell, cell)
        t1 = time.perf_counter()
        _, res = nsof.simulate_frames(comp, n_sub_steps=a.sub_steps, ctx=ctx)
        t2 = time.perf_counter()
        rec.update(host_process_images_ms=round((t1 - t0) * 1e3, 2), host_simulate_frames_ms=round((t2 - t1) * 1e3, 3),
                   host_chain_ms=round((t2 - t0) * 1e3, 2), host_chain_over_join=round((t2 - t0) / t_join, 2),
                   compress_bit_identical=bool(np.array_equal(grids.cpu().numpy(), comp)),
                   stack_bit_identical=bool(np.array_equal(stack.cpu().numpy(), 1.0 / res[1:])))
    ctx.close()
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
