"""GPU: the three entries that take per-pixel parameter planes refuse the same plane lists -- ``nsof_accum_set_param_maps``
(one array, float32 [H][W]), ``nsof_accum_trials_dev`` (T trials, float32 [T][H][W]) and ``nsof_accum_frames_f64_maps_dev``
(T trials, float64 [T][H][W]) share one host check (``plane_set_of``, csrc/accum_model.h).  Each entry is driven through the
raw C binding (Python's own checks would refuse most of these lists first) with the same bad lists; every refusal is
``NSOF_EINVAL`` with a message naming the key and -- where a value is at fault -- trial, row, column and value, leaves the
device outputs untouched, and the uniform run that follows on the same context gives the bits it gave before.

Two lists concern ``ln(Roff / Ron)``.  A Ron plane of 1e-30 against a Roff plane of 1e30 is accepted (the quotient 1e60 is a
finite double): the positive control.  A scalar Ron of 1e-300 with a Roff plane of 1e30 is refused -- but by the check of the
scalars, which comes first and finds that Ron rounds to the float32 0 (``nsof_accum_create_p`` refuses to make such an
array at all), so the message names Ron and no position.  No float32 plane can make the quotient overflow (Ron must be a
positive float32, Roff a finite one: at most 3.4e38 / 1.4e-45); it can underflow, through a scalar Roff of 1e-300, which the
scalars' check accepts: that list reaches the quotient test in all three entries and is refused naming the position."""
import ctypes as C

import numpy as np
import pytest

import accum_params_ref as R
from test_accum_trials_cpu import EV

pytestmark = pytest.mark.gpu

F = np.float32
H, W, GRID, T = 6, 8, (2, 3), 2
ACTIVE_V, SILENT_V = -6.0, 0.0
FRAME_DT, FRAME_SUB, FRAME_TH = 5e-4, 2, (0.7, 1.5)
SENTINEL = -77.0
KEY = {k: i for i, k in enumerate(R.KEYS)}


class Entry:
    """One entry point: ``call(keys, planes, counts, params)`` -> (status, message, results or None)."""

    def __init__(self, name, nsof_lib, ctx, torch_dev):
        import torch
        self.name, self.nsof, self.ctx, self.torch, self.dev = name, nsof_lib, ctx, torch, torch_dev
        self.shape = GRID if name == "frames" else (H, W)
        self.dtype = np.float64 if name == "frames" else F
        self.trials = 1 if name == "single" else T
        self.imgs = torch.from_numpy(np.random.default_rng(3).random((2,) + GRID)).to(torch_dev)

    def plane(self, key, trials=None):
        return np.full((self.trials if trials is None else trials,) + self.shape, R.DEFAULT[key], self.dtype)

    def _error(self):
        return (self.ctx._lib.nsof_last_error(self.ctx.ptr) or b"").decode()

    def call(self, keys, planes, counts, params=None):
        from nsof import _lib
        from nsof.accumulator import Accumulator, accum_params, slice_index_array
        n = len(keys)
        ckeys, ccounts = (C.c_int * max(n, 1))(*keys), (C.c_int * max(n, 1))(*counts)
        cplanes = (C.c_void_p * max(n, 1))(*[None if a is None else a.ctypes.data for a in planes])
        lib, torch = self.ctx._lib, self.torch
        idx = slice_index_array(EV[3], 1000)
        if self.name == "single":
            try:
                acc = Accumulator(H, W, 1, "split", ACTIVE_V, SILENT_V, ctx=self.ctx, params=params)
            except self.nsof.error as e:
                return e.status, str(e), None
            try:
                rc = lib.nsof_accum_set_param_maps(acc._p, n, ckeys, cplanes)
                if rc:
                    return rc, self._error(), None
                acc.step(*EV, idx)
                return rc, "", [acc.w(0), acc.resistance(0)]
            finally:
                acc.close()
        ap = accum_params(params)
        if self.name == "trials":
            outs = [torch.full((1, T, H, W), SENTINEL, dtype=torch.float32, device=self.dev) for _ in range(2)]
            torch.cuda.synchronize(self.dev)
            rc = lib.nsof_accum_trials_dev(self.ctx.ptr, H, W, 1, 0, ACTIVE_V, SILENT_V, C.byref(ap), 1, EV[0].ctypes.data,
                                           EV[1].ctypes.data, EV[2].ctypes.data, EV[3].ctypes.data, idx.ctypes.data, len(idx) - 1, 1, 0,
                                           1.0, T, n, ckeys, cplanes, ccounts, outs[0].data_ptr(), outs[1].data_ptr(), None)
        else:
            outs = [torch.full(s, SENTINEL, dtype=torch.float64, device=self.dev) for s in ((T,) + GRID, (T, 2) + GRID, (T, 1) + GRID)]
            torch.cuda.synchronize(self.dev)
            rc = lib.nsof_accum_frames_f64_maps_dev(self.ctx.ptr, self.imgs.data_ptr(), 2, GRID[0], GRID[1], FRAME_DT, FRAME_SUB,
                                                    FRAME_TH[0], FRAME_TH[1], 1.0, C.byref(ap), T, n, ckeys, cplanes, ccounts,
                                                    outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr())
        self.ctx.synchronize()
        got = [o.cpu().numpy() for o in outs]
        if rc:
            assert rc != _lib.NSOF_OK and all((g == SENTINEL).all() for g in got), (self.name, "a refused call wrote its outputs")
            return rc, self._error(), None
        return rc, "", got

    def uniform(self):
        rc, msg, got = self.call([], [], [])
        assert rc == 0, msg
        return got


@pytest.fixture(params=["single", "trials", "frames"])
def entry(request, nsof_lib, ctx, torch_dev):
    return Entry(request.param, nsof_lib, ctx, torch_dev)


def same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_the_three_entries_refuse_the_same_plane_lists(entry):
    from nsof import _lib
    e = entry
    t, r, c = e.trials - 1, 1, 2                         # the known position: the last trial, row 1, column 2
    where = f"trial {t}, row {r}, column {c}"

    def spoiled(key, value):
        a = e.plane(key)
        a[t, r, c] = value
        return a
    koff, kon = e.plane("koff"), e.plane("kon")
    n_t = e.trials
    # (what, keys, planes, trial counts, scalars, what the message holds)
    lists = [("key -1", [-1], [koff], [n_t], None, ["key -1"]),
             ("key 13", [13], [koff], [n_t], None, ["key 13"]),
             ("a NULL plane", [KEY["koff"]], [None], [n_t], None, ["koff", "NULL"]),
             ("a key given twice", [KEY["kon"], KEY["kon"]], [kon, kon], [n_t, n_t], None, ["kon", "twice"]),
             ("NaN in koff", [KEY["koff"]], [spoiled("koff", np.nan)], [n_t], None, ["koff", where, "nan"]),
             ("+inf in koff", [KEY["koff"]], [spoiled("koff", np.inf)], [n_t], None, ["koff", where, "inf"]),
             ("von = -0.125", [KEY["von"]], [spoiled("von", -0.125)], [n_t], None, ["von", where, "-0.125"]),
             ("son = 1.5", [KEY["son"]], [spoiled("son", 1.5)], [n_t], None, ["son", where, "1.5"]),
             # refused by the scalars' check, which comes first: no position (see the module's docstring)
             ("scalar Ron = 1e-300, Roff plane of 1e30", [KEY["Roff"]], [np.full_like(koff, 1e30)], [n_t], dict(R.DEFAULT, Ron=1e-300),
              ["Ron"]),
             ("scalar Roff = 1e-300, Ron = 1e30 at one pixel", [KEY["Ron"]], [spoiled("Ron", 1e30)], [n_t], dict(R.DEFAULT, Roff=1e-300),
              ["Ron / Roff", where])]
    if e.name != "single":                               # the two entries that have a trial axis
        lists.append(("a plane of 3 trials where 2 run", [KEY["koff"]], [e.plane("koff", 3)], [3], None, ["koff", "3 trials"]))
    before = e.uniform()
    assert all(np.isfinite(a).all() for a in before)
    for what, keys, planes, counts, scalars, holds in lists:
        rc, msg, got = e.call(keys, planes, counts, scalars)
        assert rc == _lib.NSOF_EINVAL and got is None, (e.name, what, rc, msg)
        assert all(h in msg for h in holds), (e.name, what, msg)
        assert same(e.uniform(), before), (e.name, what)
    # the positive control: each value in its domain and a finite quotient, 1e60
    rc, msg, got = e.call([KEY["Ron"], KEY["Roff"]], [np.full_like(koff, 1e-30), np.full_like(koff, 1e30)], [n_t, n_t])
    assert rc == 0, (e.name, msg)
    assert all(np.isfinite(a).all() for a in got), e.name
    assert same(e.uniform(), before)
