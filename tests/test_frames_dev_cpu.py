"""CPU: the host pieces of the frame-driven gating path on the device -- the C restatement of the Lanczos-3 tap tables
against the NumPy mirror, and the refusals of the Python entries that need no GPU."""
import ctypes as C

import numpy as np
import pytest


def _c_contributions(lib, in_len, out_len):
    taps = C.c_int(-1)
    assert lib.nsof_lanczos3_contributions(in_len, out_len, None, None, 0, C.byref(taps)) == 0
    n = taps.value
    wts = np.full((out_len, n), np.nan, np.float64)
    ind = np.full((out_len, n), -1, np.int32)
    assert lib.nsof_lanczos3_contributions(in_len, out_len, wts.ctypes.data, ind.ctypes.data, n, C.byref(taps)) == 0
    assert taps.value == n
    return wts, ind


@pytest.mark.parametrize("in_len,out_len", [(161, 4), (801, 4), (7, 1), (300, 3), (64, 8), (45, 45), (1920, 24)])
def test_contributions_match_the_mirror(nsof_lib, in_len, out_len):
    """Tap count and mirrored indices equal; weights within 1e-13, the bound tests/test_frames.py uses between the mirror
    and a scalar restatement (the mirror normalises with NumPy's pairwise row sum, the restatement with a running one)."""
    from nsof import _lib, frames
    wts, ind = _c_contributions(_lib.load(), in_len, out_len)
    ref_w, ref_i = frames._contributions(in_len, out_len, out_len / in_len)
    assert wts.shape == ref_w.shape
    assert np.array_equal(ind, ref_i)
    assert ind.min() >= 0 and ind.max() < in_len
    assert np.abs(wts - ref_w).max() < 1e-13


def test_contributions_refusals(nsof_lib):
    from nsof import _lib
    lib = _lib.load()
    taps = C.c_int(0)
    assert lib.nsof_lanczos3_contributions(0, 1, None, None, 0, C.byref(taps)) == _lib.NSOF_EINVAL
    assert lib.nsof_lanczos3_contributions(8, 0, None, None, 0, C.byref(taps)) == _lib.NSOF_EINVAL
    assert lib.nsof_lanczos3_contributions(8, 2, None, None, 0, None) == _lib.NSOF_EINVAL
    wts = np.full((4, 64), 7.0)
    ind = np.full((4, 64), 7, np.int32)
    assert lib.nsof_lanczos3_contributions(161, 4, wts.ctypes.data, None, 64, C.byref(taps)) == _lib.NSOF_EINVAL
    assert lib.nsof_lanczos3_contributions(161, 4, wts.ctypes.data, ind.ctypes.data, 64, C.byref(taps)) == _lib.NSOF_EINVAL
    assert taps.value > 64 and (wts == 7.0).all() and (ind == 7).all()   # too little room: the count, nothing written


def test_new_entries_refuse_a_null_context(nsof_lib):
    from nsof import _lib
    lib = _lib.load()
    w = np.ones((1, 1))
    i = np.zeros((1, 1), np.int32)
    assert lib.nsof_frames_compress_u8_dev(None, 1, 64, 1, 1, 1, 1, 1, 1, w.ctypes.data, i.ctypes.data, 1, w.ctypes.data,
                                           i.ctypes.data, 1, 64) == _lib.NSOF_EINVAL
    assert lib.nsof_accum_frames_f64_dev(None, 64, 2, 1, 1, 5e-4, 10, 0.7, 1.5, 1.0, 64, 64, None) == _lib.NSOF_EINVAL


def test_python_refusals_without_a_gpu(nsof_lib):
    """A host tensor, a NumPy array and the wrong dtype are refused before the library (or a device) is touched."""
    import torch
    from nsof import frames, pipeline
    from nsof.gating import GatingConfig
    for bad in (torch.zeros((2, 16, 16), dtype=torch.uint8), np.zeros((2, 16, 16), np.uint8),
                torch.zeros((2, 16, 16), dtype=torch.float32)):
        with pytest.raises(nsof_lib.error) as e:
            frames.process_images_dev(bad, 4, 4)
        assert isinstance(e.value, ValueError)
    for bad in (torch.zeros((2, 4, 4), dtype=torch.float64), np.zeros((2, 4, 4))):
        with pytest.raises(nsof_lib.error):
            nsof_lib.simulate_frames_dev(bad)
    with pytest.raises(nsof_lib.error):
        pipeline.gating_stack_from_frames_dev(torch.zeros((3, 16, 16, 3), dtype=torch.uint8), GatingConfig(MEMSIZE=4))
    assert nsof_lib.process_images_dev is frames.process_images_dev
    assert nsof_lib.gating_stack_from_frames_dev is pipeline.gating_stack_from_frames_dev
