"""Live cross-check of the Gaussian window (flags = 256) against the real cv2 wherever it is importable.

The opencv-python wheel is not installed in the build image or on the GPU boxes, so these tests normally SKIP and the parity
claim for the flag stays "vs the float32 restatement of tests/farneback_gauss.py; parity with cv2 unpinned" (DESIGN.md
section 2: a wheel's SIMD build may fuse the multiply-adds of the two blur passes).  On a machine that has cv2 they hold
the restatement and the HIP path to the bar of tests/test_cv2_crosscheck.py.
"""
import numpy as np
import pytest

cv2 = pytest.importorskip("cv2", reason="opencv-python is not installed here: parity with cv2 stays unpinned")

import farneback_gauss as G  # noqa: E402
from test_cv2_crosscheck import TOL, A, B, C, _pairs, _pyramid_variant  # noqa: E402

SETS = [dict(kw, flags=cv2.OPTFLOW_FARNEBACK_GAUSSIAN) for kw in (A, B, C)]


@pytest.mark.parametrize("kw", SETS, ids="ABC")
def test_restatement_vs_cv2(oracle, kw):
    cv2.setNumThreads(1)
    v = _pyramid_variant(oracle)
    oracle.set_pyr_fma(bool(v))
    try:
        for prev, nxt in _pairs():
            want = cv2.calcOpticalFlowFarneback(prev, nxt, None, **kw)
            got = G.farneback_gauss(np.ascontiguousarray(prev), np.ascontiguousarray(nxt), *kw.values())
            assert got.shape == want.shape and want.dtype == np.float32
            assert float(np.abs(got - want).max()) < TOL, f"pyramid variant {v}"
    finally:
        oracle.set_pyr_fma(False)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", SETS, ids="ABC")
def test_hip_vs_cv2(nsof_lib, ctx, kw):
    from nsof import _lib
    from oracle import oracle as O  # noqa: N812
    pairs = list(_pairs())
    ctx.set_option(_lib.OPT_PYR_FMA, 1 if _pyramid_variant(O) == 1 else 0)   # the variant this wheel executes
    try:
        batch = nsof_lib.farneback_pairs(pairs, kw, ctx=ctx)
        for (prev, nxt), fb in zip(pairs, batch):
            want = cv2.calcOpticalFlowFarneback(prev, nxt, None, **kw)
            got = nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, **kw, ctx=ctx)
            assert float(np.abs(got - want).max()) < TOL
            assert np.array_equal(fb, got)
    finally:
        ctx.set_option(_lib.OPT_PYR_FMA, 0)
