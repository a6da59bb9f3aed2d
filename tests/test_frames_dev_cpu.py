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


def _kernel_constant(name):
    """An integer `constexpr int NAME = value;` of csrc/frames_kernels.hip."""
    import os
    import re
    from conftest import PKG
    with open(os.path.join(PKG, "csrc", "frames_kernels.hip")) as f:
        return int(re.search(rf"constexpr int {name} = (\d+);", f.read()).group(1))


def _compress_geometry(h, w, m, n):
    """What nsof_frames_compress_u8_dev launches for an h x w frame compressed by n, m -> (rows_first, x tiles and last x
    tile's width of k_resize_rows, y tiles and last y tile's height of k_resize_cols, taps y, taps x), with the tile
    sizes the issue of this coverage names (256 columns, 64 rows)."""
    from nsof import frames
    out_h, out_w = h // n, w // m
    rows_first = out_h * w <= out_w * h                 # the smaller scale first, rows on a tie
    other_rows = w if rows_first else out_w             # the axis the rows pass does not resize
    other_cols = out_h if rows_first else h
    taps_y = frames._contributions(h, out_h, out_h / h)[0].shape[1]
    taps_x = frames._contributions(w, out_w, out_w / w)[0].shape[1]
    return (rows_first, -(-other_rows // 256), (other_rows - 1) % 256 + 1, -(-other_cols // 64), (other_cols - 1) % 64 + 1,
            taps_y, taps_x)


# the cases that give more than one tile: (rows first, x tiles, last x tile, y tiles, last y tile, taps y, taps x)
TILED_CASES = {
    (130, 600, 2, 2): (True, 3, 88, 2, 1, 12, 12),
    (65, 257, 1, 1): (True, 2, 1, 2, 1, 5, 5),
    (64, 256, 1, 1): (True, 1, 256, 1, 64, 5, 5),
    (200, 520, 2, 1): (False, 2, 4, 4, 8, 5, 12),
    (150, 1030, 4, 2): (False, 2, 1, 3, 22, 12, 25),
    (130, 2600, 10, 1): (False, 2, 4, 3, 2, 5, 60),
    (700, 66, 1, 10): (True, 1, 66, 2, 6, 60, 5),
}


def test_compress_cases_cover_many_tiles_on_both_axes():
    """The GPU test's COMPRESS_CASES, recomputed from the shapes and the mirror's tap tables: both kernels run with more
    than one tile in either pass order, with a last tile of one element, and the LDS staging takes a second round in a
    second row tile.  An edit of the list that loses one of these fails here, without a GPU."""
    from test_frames_dev_gpu import COMPRESS_CASES
    assert (_kernel_constant("ROWS_BLOCK"), _kernel_constant("COLS_ROWS"), _kernel_constant("COLS_TAPS")) == (256, 64, 32)
    geo = {case: _compress_geometry(*case) for case in COMPRESS_CASES}
    for case, want in TILED_CASES.items():
        assert geo[case] == want, (case, geo[case])
    # the pass order of the mirror is the one computed here
    for (h, w, m, n), g in geo.items():
        assert g[0] == ((h // n) / h <= (w // m) / w), (h, w, m, n)
    g = list(geo.values())
    for rows_first in (True, False):
        assert any(c[0] == rows_first and c[1] > 1 for c in g), ("more than one x tile, rows first:", rows_first)
        assert any(c[0] == rows_first and c[3] > 1 for c in g), ("more than one y tile, rows first:", rows_first)
    assert any(c[1] > 1 and c[2] == 1 for c in g), "a last x tile of one column"
    assert any(c[3] > 1 and c[4] == 1 for c in g), "a last y tile of one row"
    assert any(c[1] == 1 and c[2] == 256 for c in g) and any(c[3] == 1 and c[4] == 64 for c in g), "one full tile"
    assert any(c[6] > 32 and c[3] > 1 for c in g), "a columns pass with a second staging round and a second row tile"


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
