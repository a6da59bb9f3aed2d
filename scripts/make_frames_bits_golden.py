#!/usr/bin/env python3
"""Record the frame-driven array run's bits: tests/golden/frames_run_bits.npz (read by tests/test_frames_bits_gpu.py).

    python scripts/make_frames_bits_golden.py [--out tests/golden/frames_run_bits.npz]

Needs a GPU.  Uses the public Python API only -- ``nsof.simulate_frames`` on host arrays, no maps -- so it runs unchanged
on any commit that has that function; the committed file was written at the last commit whose host entry launched one
kernel per frame pair (k_frame_step), the oldest statement of the contract.

Stored: the input frames per grid (``imgs_<H>x<W>``: the test does not depend on NumPy's generator stream), and per case
``w_<case>`` / ``res_<case>``; ``cases`` is a JSON list of {name, grid, n_frames, th1, th2, device}.

  inputs      those of tests/test_frames_dev_gpu.py::_array_case: grids 1x1, 4x4, 6x8, 13x24, five frames, seed H * 100 + W,
              dt 5e-4, 50 sub-steps
  thresholds  (th1, th2) = (0.7, 1.5), (2.0, 1.5), (8.0, 1.5); only th1 = 8.0 puts cells of these inputs in the dead
              zone [voff, von]
  devices     the default one (the FITTED instantiation) on every grid; tests/accum_params_ref.py's SETS["alpha"] (the
              pow(a, alpha) arm) and SETS["wide"] on 4x4 and 13x24
  edge cases  n_frames = 1 and 2 on 4x4, the default device

Asserted here (and again by the test, on the stored frames): at th1 = 8.0 every grid of at least 4x4 has a (pair, cell)
in each of the regimes V < voff, V > von, voff <= V <= von, for every device run on it; and every case's ``res``
holds more than two distinct values (but a run of one frame: it holds r0 alone)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "neuromorphic-spatiotemporal-optical-flow_amd"), os.path.join(ROOT, "tests")]

GRIDS = [(1, 1), (4, 4), (6, 8), (13, 24)]
THRESHOLDS = [(0.7, 1.5), (2.0, 1.5), (8.0, 1.5)]
DEVICE_GRIDS = {"default": GRIDS, "alpha": [(4, 4), (13, 24)], "wide": [(4, 4), (13, 24)]}
DT, N_SUB = 5e-4, 50


def make_frames(np, grid):
    rng = np.random.default_rng(grid[0] * 100 + grid[1])
    base = rng.random(grid)
    step = rng.choice([0.0, 0.002, 0.01, 0.3], size=(5,) + grid) * rng.standard_normal((5,) + grid)
    return np.clip(base + step, 0.0, 1.0)


def regime_counts(np, imgs, th1, voff, von):
    """(off, on, dead): how many (pair, cell) drives fall below voff, above von, inside [voff, von]."""
    d = np.abs(imgs[:-1] * 256 - imgs[1:] * 256)
    v = np.where(d > th1, (d + 4) * 0.75, (d - 5.5) * 0.6)
    v = np.where(v > 0, -(0.3 * v + 0), np.where(v < 0, -(3 * v + -3), 0.0))
    return int((v < voff).sum()), int((v > von).sum()), int(((v >= voff) & (v <= von)).sum())


def case_list():
    cases = []
    for device, grids in DEVICE_GRIDS.items():
        for grid in grids:
            for th1, th2 in THRESHOLDS:
                cases.append(dict(name=f"{device}_{grid[0]}x{grid[1]}_th{th1}", grid=list(grid), n_frames=5, th1=th1, th2=th2,
                                  device=device))
    for n in (1, 2):
        for th1, th2 in THRESHOLDS:
            cases.append(dict(name=f"default_4x4_th{th1}_n{n}", grid=[4, 4], n_frames=n, th1=th1, th2=th2, device="default"))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "frames_run_bits.npz"))
    a = ap.parse_args()
    os.environ.setdefault("NSOF_SKIP_BUILD", "1")
    import numpy as np

    import accum_params_ref as R  # noqa: N812
    import nsof
    devices = {"default": None, "alpha": R.SETS["alpha"]["params"], "wide": R.SETS["wide"]["params"]}
    ctx = nsof.Context(0)
    store = {f"imgs_{g[0]}x{g[1]}": make_frames(np, g) for g in GRIDS}
    cases = case_list()
    for c in cases:
        imgs = store[f"imgs_{c['grid'][0]}x{c['grid'][1]}"][:c["n_frames"]]
        params = devices[c["device"]]
        w, res = nsof.simulate_frames(imgs, DT, N_SUB, c["th1"], c["th2"], ctx=ctx, params=params)
        assert w.shape == tuple(c["grid"]) and res.shape == (c["n_frames"],) + tuple(c["grid"])
        if c["n_frames"] > 1:
            assert np.unique(res).size > 2, c["name"]
        if c["n_frames"] == 5:
            p = params or nsof.PARAMS
            counts = regime_counts(np, imgs, c["th1"], p["voff"], p["von"])
            print(c["name"], "off / on / dead:", counts)
            if c["th1"] == 8.0 and c["grid"][0] >= 4:
                assert min(counts) > 0, (c["name"], counts)
        store[f"w_{c['name']}"] = w
        store[f"res_{c['name']}"] = res
    ctx.close()
    store["cases"] = np.array(json.dumps(cases))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez_compressed(a.out, **store)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(cases)} cases")


if __name__ == "__main__":
    main()
