#!/usr/bin/env python3
"""A/B of two libnsof builds on the pyramid and flow-resample stages: alternating runs of scripts/stage_bench.py (a fresh
process each, the library chosen by NSOF_LIB), the same inputs for both, every output compared byte for byte (SHA-1).

    python scripts/ab_pyramid.py --parent nsof/libnsof_parent.so [--rounds 5] [--out profiles/pyramid_refactor.json]

Criterion per stage: the new library's median lies inside the parent's min-max over the rounds.  Exit status 2 if an
output differs or a median lies above the parent's maximum (1: a run itself failed)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd", "nsof", "libnsof.so")
# name -> stage_bench.py arguments, and the kernels the configuration reaches
CASES = {
    "1080p_0.5": ("--stages prep0,prep1,prep2,prep3,upsample",
                  "k_prep_same3_vec, k_prep_decim<2,4,8>, k_flow_upsample_walk"),
    "1080p_0.6": ("--stages prep1,prep2,prep3,upsample --pyr-scale 0.6", "k_prep_walk<3,5,9>, k_flow_upsample_walk"),
    "1916x1080_0.5": ("--stages prep1,prep2,prep3 --width 1916", "k_prep_walk<3>, k_prep_walk<9>, k_prep_rows/cols<19>"),
    "1080p_0.6_f32": ("--stages prep1,prep2,prep3 --pyr-scale 0.6 --pixel-type f32", "k_prep_walk<3,5,9, float>"),
    "1916x1080_0.5_f32": ("--stages prep3 --width 1916 --pixel-type f32", "k_prep_rows<19, float>, k_prep_cols<19>"),
    "1080p_0.6_u16": ("--stages prep1,prep2,prep3 --pyr-scale 0.6 --pixel-type u16", "k_prep_walk<3,5,9, uint16_t>"),
    "1080p_0.3": ("--stages prep1 --pyr-scale 0.3", "k_prep_tiled<0> (7 taps at run time)"),
    "480x270_0.4": ("--stages prep3 --pyr-scale 0.4 --width 480 --height 270 --pairs 8", "k_prep_naive (37 taps)"),
    "8192x3_0.42": ("--stages prep1 --pyr-scale 0.42 --width 8192 --height 3 --pairs 512", "uniform k_prep_direct<3>"),
    "240x136_0.5": ("--stages upsample --width 240 --height 136", "k_flow_upsample2x2"),
    # work lists (this script as the worker): the prep launches of a list of 64 crops, all its levels together
    "worklist_A": ("--worklist A", "k_prep_direct<3, HET>, k_prep_tiled<9, HET>, k_prep_tiled<19, HET>"),
    "worklist_B": ("--worklist B", "k_prep_direct<3, HET>, k_prep_direct<5, HET>, k_prep_tiled<9, HET>"),
    "worklist_B_s16": ("--worklist B --pixel-type s16", "the same on int16 crops"),
    "worklist_B_f32": ("--worklist B --pixel-type f32", "the same on float32 crops"),
}


def worklist(params, pixel_type, reps=20, n=64, ch=200, cw=520):
    """Worker: 64 crops of 520x200 of two 1080p frames at positions that are not a constant step apart (so the list takes
    the work-list kernels, not the uniform driver) as one list; prints the prep time per list and the flows' SHA-1."""
    import hashlib
    sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd")]
    import nsof
    import torch
    from nsof import _lib
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    fr = torch.randint(0, 256, (2, 1080, 1920), dtype=torch.uint8, device=dev, generator=g)
    from nsof import farneback as fb
    fn = fb.farneback_pairs_dev
    if pixel_type == "f32":
        fr, fn = fr.float(), fb.farneback_pairs_f32_dev
    elif pixel_type == "s16":
        fr, fn = (fr.to(torch.int32) * 100 - 12000).to(torch.int16), fb.farneback_pairs_16_dev
    canvas = torch.zeros((n, ch, cw, 2), dtype=torch.float32, device=dev)
    flows = [canvas[i] for i in range(n)]
    p = {"A": nsof.farneback.PARAMS_A, "B": nsof.farneback.PARAMS_B}[params]
    origins = [((7 * i * i + 3 * i) % (1080 - ch), (37 * i + (i * i) % 11) % (1920 - cw)) for i in range(n)]
    pairs = [(fr[0, y:y + ch, x:x + cw], fr[1, y:y + ch, x:x + cw]) for (y, x) in origins]
    ctx = nsof.Context(0)
    for _ in range(3):
        fn(pairs, flows, p, ctx=ctx)
    ctx.synchronize()
    ctx.prof_enable(_lib.K_PREP)
    for _ in range(reps):
        fn(pairs, flows, p, ctx=ctx)
    ctx.synchronize()
    ms, cnt = ctx.prof_collect(_lib.K_PREP)
    ctx.prof_enable()
    print(f"prep_list {ms * 1e3 / reps:9.1f} us/launch  ({cnt // reps} launches per list)", flush=True)
    print(f"digest prep_list {hashlib.sha1(canvas.cpu().numpy().tobytes()).hexdigest()}", flush=True)
    ctx.close()


def run(lib, args):
    env = dict(os.environ, NSOF_LIB=lib, NSOF_SKIP_BUILD="1")
    if args.startswith("--worklist"):
        cmd = [sys.executable, os.path.abspath(__file__)] + args.split()
    else:
        cmd = [sys.executable, os.path.join(ROOT, "scripts", "stage_bench.py"), "--digest"] + args.split()
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, check=True).stdout
    us, sha = {}, {}
    for line in out.splitlines():
        f = line.split()
        if len(f) > 2 and f[2] == "us/launch":
            us[f[0]] = float(f[1])
        elif f and f[0] == "digest":
            sha[f[1]] = f[2]
    return us, sha


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the library to compare against (same ABI)")
    ap.add_argument("--worklist", choices=["A", "B"], help="worker mode: one work-list measurement with this parameter set")
    ap.add_argument("--pixel-type", choices=["u8", "f32", "s16"], default="u8")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worklist:
        worklist(a.worklist, a.pixel_type)
        return 0
    res, bad = {}, []
    for name in a.cases.split(","):
        args, reaches = CASES[name]
        t = {"parent": {}, "new": {}}
        for _ in range(a.rounds):
            shas = {}
            for which, lib in (("parent", os.path.abspath(a.parent)), ("new", NEW)):
                us, shas[which] = run(lib, args)
                for st, v in us.items():
                    t[which].setdefault(st, []).append(v)
            if shas["parent"] != shas["new"] or not shas["new"]:
                bad.append(f"{name}: outputs differ {shas}")
        for st in t["new"]:
            p, nw = t["parent"][st], t["new"][st]
            row = {"reaches": reaches, "parent_us": p, "new_us": nw, "parent_min_max": [min(p), max(p)],
                   "new_median": statistics.median(nw), "same_bytes": not any(b.startswith(name + ":") for b in bad)}
            row["inside"] = min(p) <= row["new_median"] <= max(p)
            if row["new_median"] > max(p):
                bad.append(f"{name}/{st}: median {row['new_median']} above the parent's max {max(p)}")
            res[f"{name}/{st}"] = row
            print(f"{name + '/' + st:28s} parent {min(p):8.1f} .. {max(p):8.1f}  new median {row['new_median']:8.1f}  "
                  f"{'inside' if row['inside'] else ('BELOW' if row['new_median'] < min(p) else 'ABOVE')}", flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"what": "us per launch, scripts/stage_bench.py (32 pairs unless the case says otherwise), parent "
                               "and new library alternating, one process per run", "rounds": a.rounds, "stages": res,
                       "failures": bad}, f, indent=1)
    for b in bad:
        print("FAIL", b)
    return 2 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
