"""CPU: the oracle's float -> int conversions at NaN, +-inf and out-of-range values.

cvFloor in the matrix update and cvRound in the remap are C casts that are undefined for such values; the oracle states
what an x86-64 cv2 build returns instead (oracle/farneback_ref.c cv_floor_f, oracle/warp_ref.c cv_round_f), and the
device kernels return the same (tests/test_extreme_content_gpu.py).  Consequences pinned here:

* matrix update: a non-finite or out-of-range sample position takes the out-of-image branch, so M channels 0-2 (which
  do not depend on the flow there) stay finite;
* remap: NaN, +-inf and any map whose x32 product leaves the int range sample at (-32768, ...): BORDER_CONSTANT writes
  the border value, BORDER_REPLICATE the first column / row with a zero fraction."""
import numpy as np
import pytest

import farneback_f64 as F

BAD = [np.nan, np.inf, -np.inf, 1e10, -1e10]


def _flows(h, w):
    """Bad values at interior and border pixels, in dx, dy or both; the rest a small finite flow."""
    rng = np.random.default_rng(1)
    flow = (rng.standard_normal((h, w, 2)) * 0.7).astype(np.float32)
    spots = [(h // 2, w // 2), (0, 0), (h - 1, w - 1), (2, w - 3), (h // 2, 0), (h - 2, w // 3), (6, 6)]
    for i, (y, x) in enumerate(spots):
        for j, v in enumerate(BAD):
            yy, xx = (y + j) % h, (x + 2 * j) % w
            if i % 3 == 0:
                flow[yy, xx] = (v, v)
            elif i % 3 == 1:
                flow[yy, xx, 0] = v
            else:
                flow[yy, xx, 1] = v
    return flow


def test_update_matrices_nonfinite_flow_takes_out_of_image_branch(oracle):
    h, w = 23, 31
    img = (np.random.default_rng(2).random((h, w)) * 255).astype(np.float32)
    R0 = oracle.polyexp(img, 5, 1.1)
    R1 = oracle.polyexp(np.roll(img, 2, axis=0), 5, 1.1)
    flow = _flows(h, w)
    M = oracle.update_matrices(R0, R1, flow)
    bad = ~np.isfinite(flow).all(axis=-1) | (np.abs(flow) > 1e9).any(axis=-1)
    assert bad.sum() >= 30
    # channels 0-2 at a bad pixel: the out-of-image values r4 = R0_2, r5 = R0_3, r6 = R0_4 / 2 times the border scale
    s = F.border_scale(w, h).astype(np.float32)
    r4, r5, r6 = R0[..., 2] * s, R0[..., 3] * s, R0[..., 4] * np.float32(0.5) * s
    want = np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6], axis=-1)
    assert np.isfinite(M[..., :3]).all()
    assert np.allclose(M[bad][:, :3], want[bad], rtol=1e-5, atol=1e-30)
    # every finite pixel is still the float64 reference's
    ok = ~bad
    ref, tol = F.update_matrices(R0, R1, np.where(bad[..., None], 0, flow).astype(np.float32))
    assert F.within(M[ok], ref[ok], tol[ok])[0]


# NaN, +-inf, +-1e10 and the first map values past the int range on either side (2^26 * 32 = 2^31)
REMAP_BAD = BAD + [2.0 ** 26, -2.0 ** 26 - 64]


@pytest.mark.parametrize("border", [0, 1])
def test_remap_nonfinite_maps_sample_at_int_min(oracle, border):
    rng = np.random.default_rng(3)
    sh, sw = 9, 13
    src = rng.integers(1, 255, (sh, sw), dtype=np.uint8).astype(np.int64)
    n = len(REMAP_BAD)
    mx = np.full((3, n + 1), 2.25, np.float32)
    my = np.full((3, n + 1), 3.5, np.float32)
    for j, v in enumerate(REMAP_BAD + [2.0 ** 26 - 4]):   # the last column: still in range, far right / below
        mx[0, j] = v                       # x bad, y = 3.5
        my[1, j] = v                       # y bad, x = 2.25
        mx[2, j] = my[2, j] = v            # both bad
    got = oracle.remap_linear(src.astype(np.uint8), mx, my, border, 7).astype(np.int64)
    if border == 0:                        # the 2x2 footprint at x or y = -32768 misses the source: the border value
        assert (got[:, :n] == 7).all() and (got[:, n] == 7).all()
        return
    # BORDER_REPLICATE, fraction 0 on the bad axis: column 0 / row 0 (15-bit weights, rounded half up)
    col0 = (src[3, 0] * 16 * 32 * 32 + src[4, 0] * 16 * 32 * 32 + (1 << 14)) >> 15
    row0 = (src[0, 2] * 24 * 32 * 32 + src[0, 3] * 8 * 32 * 32 + (1 << 14)) >> 15
    assert (got[0, :n] == col0).all(), got[0]
    assert (got[1, :n] == row0).all(), got[1]
    assert (got[2, :n] == src[0, 0]).all(), got[2]
    col_last = (src[3, -1] * 16 * 32 * 32 + src[4, -1] * 16 * 32 * 32 + (1 << 14)) >> 15
    assert got[0, n] == col_last and got[2, n] == src[-1, -1]
