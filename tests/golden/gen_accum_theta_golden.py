#!/opt/conda/bin/python3.9
"""Generate the golden vectors of scheme 1's event-count threshold by RUNNING THE REFERENCE ITSELF with its module knob
THETA_EVENTS set (event_mem_sim.py:33, read at :214).

Run in the build container only (the reference never travels):
    /opt/conda/bin/python3.9 tests/golden/gen_accum_theta_golden.py
Writes tests/golden/accum_theta_v1.npz: the two event streams and, per threshold, the reference's w_final and the kept
snapshots (data only, no reference source).  Keys: ``{stream}_x / _y / _p / _t / _active_v / _silent_v / _thetas``,
``{stream}_n_snapshots``, ``snap_idx`` and ``{stream}_th{theta}_w_final / _resistances`` for stream in ("dead", "leak").
"""
import tempfile
from pathlib import Path

import h5py
import numpy as np

from gen_accum_golden import ems, make_stream   # stubs cv2 and imports the reference module

OUT = Path(__file__).resolve().parent
KEEP = (0, 1, -1)
SLICE_US = 1000


def run(stream, theta, active_v, silent_v):
    x, y, p, t = stream
    ems.THETA_EVENTS = theta
    with tempfile.TemporaryDirectory() as d:
        h5 = Path(d) / "s.hdf5"
        with h5py.File(h5, "w") as f:
            g = f.create_group("/CD/events")
            g.create_dataset("x", data=x, dtype=np.int16)
            g.create_dataset("y", data=y, dtype=np.int16)
            g.create_dataset("p", data=p, dtype=np.int8)
            g.create_dataset("t", data=t, dtype=np.int64)
        ems.simulate(h5, version=1, slice_us=SLICE_US, active_v=active_v, silent_v=silent_v, save_video=False)
        a = np.load(h5.with_suffix(".V1.npz"))
        return a["w_final"], a["resistances"]


def main():
    cases = {
        "dead": (make_stream(21, 64, 48, 20000, 100_000, (0, 1)), (2, 3, 5), -6.0, 0.0),
        # silent voltage outside the dead zone: every pixel updates every slice
        "leak": (make_stream(11, 64, 48, 6000, 200_000, (0, 1)), (2, 3), -8.0, 0.5),
    }
    out = dict(snap_idx=np.array(KEEP), slice_us=SLICE_US)
    for name, (stream, thetas, active_v, silent_v) in cases.items():
        x, y, p, t = stream
        out.update({f"{name}_x": x, f"{name}_y": y, f"{name}_p": p, f"{name}_t": t, f"{name}_thetas": np.array(thetas),
                    f"{name}_active_v": np.float32(active_v), f"{name}_silent_v": np.float32(silent_v)})
        for th in thetas:
            w, res = run(stream, th, active_v, silent_v)
            out[f"{name}_n_snapshots"] = res.shape[0]
            out[f"{name}_th{th}_w_final"] = w
            out[f"{name}_th{th}_resistances"] = res[list(KEEP)]
            print(name, "theta", th, "snapshots", res.shape[0], "pixels moved", int((w != np.float32(0.5)).sum()))
    ems.THETA_EVENTS = 1
    np.savez_compressed(OUT / "accum_theta_v1.npz", **out)


if __name__ == "__main__":
    main()
