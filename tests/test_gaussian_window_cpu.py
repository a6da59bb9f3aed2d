"""CPU: the NumPy restatement of the Gaussian window (tests/farneback_gauss.py), which the GPU tests compare with bit for
bit, is itself what it claims to be: normalised taps, equal flow for both parities of a window, the oracle's own
scaffolding around the iteration, upstream's lagged stripe update, and references that move on every input the GPU tests
use for whole calls."""
import numpy as np
import pytest

import farneback_gauss as G
from test_exact_paths_gpu import _frames

WHOLE_CALL_SHAPES = [(45, 200), (70, 33), (33, 70), (130, 257), (97, 131), (96, 128)]


def _gauss_params(winsize):
    return (0.5, 2, winsize, 2, 5, 1.1, G.GAUSSIAN)


def test_constants_exported(nsof_lib):
    assert nsof_lib.OPTFLOW_FARNEBACK_GAUSSIAN == 256 == G.GAUSSIAN and nsof_lib.OPTFLOW_USE_INITIAL_FLOW == 4
    assert nsof_lib.FarnebackParams(flags=256).as_kwargs()["flags"] == 256


@pytest.mark.parametrize("winsize", range(2, 66))
def test_taps_are_normalised(winsize):
    k = G.taps(winsize)
    assert k.dtype == np.float32 and k.shape == (winsize // 2 + 1,) and (k > 0).all() and (np.diff(k) < 0).all()
    total = float(k[0]) + 2 * float(k[1:].astype(np.float64).sum())
    assert abs(total - 1) < 1e-6


def test_even_and_odd_windows_agree(oracle):
    fr = _frames(45 * 1000 + 200, 2, 45, 200)
    a = G.farneback_gauss(fr[0], fr[1], *_gauss_params(14))
    b = G.farneback_gauss(fr[0], fr[1], *_gauss_params(15))
    assert np.array_equal(a, b) and np.abs(a).max() > 1


def test_box_composition_is_the_oracle(oracle):
    fr = _frames(70 * 1000 + 130, 2, 70, 130)
    params = (0.5, 2, 7, 2, 5, 1.1, 0)
    want = oracle.farneback(fr[0], fr[1], *params)
    assert np.abs(want).max() > 1
    assert np.array_equal(G.farneback_box(fr[0], fr[1], *params), want)


@pytest.mark.parametrize("winsize", [3, 8])
def test_lagged_stripe_update_is_the_whole_field_update(oracle, winsize):
    """70 x 33: stripes of max(1024 // 33, winsize) = 31 rows, so the lagged update runs twice inside the row loop."""
    from test_farneback_gpu import _level_state
    fr = _frames(70 * 1000 + 33, 2, 70, 33)
    R0, R1, flow = _level_state(oracle, fr[0], fr[1], 5, 1.1, 6)
    M = oracle.update_matrices(R0, R1, flow)
    got_flow, got_M = G.gauss_blur_solve_rows(R0, R1, flow, M, winsize, True)
    want_flow = G.gauss_blur_solve(M, winsize)
    assert np.array_equal(got_flow, want_flow)
    assert np.array_equal(got_M, oracle.update_matrices(R0, R1, want_flow))
    assert not np.array_equal(got_M, M)


@pytest.mark.parametrize("shape", WHOLE_CALL_SHAPES)
@pytest.mark.parametrize("winsize", [3, 15, 33])
def test_references_move(oracle, shape, winsize):
    """A zero or non-finite reference would let a broken kernel pass: every whole-call input of the GPU tests gives a
    finite field that exceeds a pixel somewhere."""
    h, w = shape
    fr = _frames(h * 1000 + w, 2, h, w)
    ref = G.farneback_gauss(fr[0], fr[1], *_gauss_params(winsize))
    assert ref.shape == (h, w, 2) and ref.dtype == np.float32 and np.isfinite(ref).all()
    assert np.abs(ref).max() > 1.0, float(np.abs(ref).max())
