"""CPU: the oracle's Farneback stages against the float64 reference of tests/farneback_f64.py, whole frames (borders
included) at the shapes where the stages go wrong: 1x1, one row, one column, frames smaller than the expansion's
(2n+1)^2 neighbourhood, the pyramid blur's kernel and the blur's window; every poly_n 1..10 (sigma 0 included),
every window 2..31, pyr_scale 0.3 .. 0.8 at odd sizes.  Each comparison holds the oracle to the float32 error bound the
reference derives for that stage (its module docstring).  The whole pipeline is then checked on two frames with a
known answer: constant frames give exactly zero flow, integer translations of a texture are recovered in the
interior."""
import numpy as np
import pytest

import farneback_f64 as F

SHAPES = [(1, 1), (1, 9), (9, 1), (3, 4), (5, 12), (12, 5), (17, 23), (40, 50)]
SCALES = (0.3, 0.4, 0.45, 0.5, 0.55, 0.6, 0.7, 0.8)


def _ids(shapes):
    return [f"{h}x{w}" for h, w in shapes]


def _noise(seed, shape, hi=255.0):
    return (np.random.default_rng(seed).random(shape) * hi).astype(np.float32)


def _check(got, ref_tol, what):
    ref, tol = ref_tol
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    ok, worst = F.within(got, ref, tol)
    if not ok:
        i = np.unravel_index(np.argmax(np.abs(got - ref) / np.maximum(tol, 1e-300)), got.shape)
        raise AssertionError(f"{what}: {worst:.3g} x the bound at {i}: got {got[i]!r}, float64 {ref[i]!r}, "
                             f"bound {tol[i]:.3g}")
    return worst


def _stage_inputs(seed, h, w):
    """Expansions of two noise frames and a flow that sends part of the frame outside (both signs, both axes)."""
    img = _noise(seed, (h, w))
    R0 = F.polyexp(img, 3, 1.0)[0].astype(np.float32)
    R1 = F.polyexp(np.roll(img, 1, axis=1), 3, 1.0)[0].astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    flow = (rng.standard_normal((h, w, 2)) * 1.5).astype(np.float32)
    flow[::3, ::2, 0] += np.float32(max(2, w // 3))
    flow[1::4, :, 1] -= np.float32(max(2, h // 3))
    return R0, R1, flow


# ---------------------------------------------------------------- stages
@pytest.mark.parametrize("shape", SHAPES + [(31, 45)], ids=_ids(SHAPES + [(31, 45)]))
def test_polyexp_every_radius(oracle, shape):
    """Every poly_n 1..10, with sigma 0 (cv2's default 0.3 n) and with the A/B/C sigmas, frames smaller than 2n+1."""
    img = _noise(sum(shape), shape)
    for n in range(1, 11):
        for sigma in (0.0, 1.05, 1.2, 0.3 * n + 0.7):
            _check(oracle.polyexp(img, n, sigma), F.polyexp(img, n, sigma), f"polyexp n={n} sigma={sigma}")


def test_polyexp_borders_replicate(oracle):
    """A ramp in x and y: replicate and reflect borders give different edge columns and rows by far more than the
    bound, so this pins the border mode of both passes."""
    h, w = 14, 19
    yy, xx = np.mgrid[0:h, 0:w]
    img = (3.0 * xx + 7.0 * yy + 0.25 * xx * yy).astype(np.float32)
    for n in (2, 5, 9):
        _check(oracle.polyexp(img, n, 0.0), F.polyexp(img, n, 0.0), f"polyexp ramp n={n}")


@pytest.mark.parametrize("shape", SHAPES + [(33, 47), (61, 83), (101, 77)], ids=_ids(SHAPES + [(33, 47), (61, 83),
                                                                                              (101, 77)]))
def test_pyr_level_every_scale(oracle, shape):
    """Blur + resize of an 8-bit frame at every pyr_scale and level whose size is at least 1x1 (the oracle's blur takes
    kernels up to 63 taps); kernels far wider than the frame included."""
    h, w = shape
    img = np.random.default_rng(w * 31 + h).integers(0, 256, shape, dtype=np.uint8)
    done = 0
    for ps in SCALES:
        for k in range(0, 6):
            wk, hk, ksize, _ = F.level_geometry(w, h, ps, k)
            assert (wk, hk, ksize) == oracle.level_geometry(w, h, ps, k)[:3]
            if wk < 1 or hk < 1 or ksize > 63:
                continue
            _check(oracle.pyr_level(img, ps, k), F.pyr_level(img, ps, k), f"pyr_level ps={ps} k={k}")
            done += 1
    assert done >= len(SCALES)


@pytest.mark.parametrize("src,dst", [((1, 1), (2, 2)), ((1, 3), (2, 5)), ((3, 1), (5, 2)), ((2, 2), (3, 4)),
                                     ((5, 7), (9, 11)), ((9, 16), (17, 27)), ((20, 30), (40, 60)),
                                     ((17, 23), (57, 77))])
@pytest.mark.parametrize("pyr_scale", [0.3, 0.5, 0.6, 0.8])
def test_flow_upsample(oracle, src, dst, pyr_scale):
    """The driver's coarse-to-fine step: resize_linear of the flow, then times float32(1 / pyr_scale)."""
    f = (np.random.default_rng(src[0] * 7 + dst[1]).standard_normal(src + (2,)) * 4).astype(np.float32)
    got = oracle.resize_linear(f, dst[1], dst[0]) * np.float32(1.0 / pyr_scale)
    _check(got, F.flow_upsample(f, dst[1], dst[0], pyr_scale), "flow_upsample")


@pytest.mark.parametrize("shape", SHAPES + [(11, 11), (31, 45)], ids=_ids(SHAPES + [(11, 11), (31, 45)]))
def test_update_matrices_whole_frame(oracle, shape):
    """Every pixel, the five-pixel border weights and the out-of-image branch included."""
    R0, R1, flow = _stage_inputs(shape[0] * 100 + shape[1], *shape)
    _check(oracle.update_matrices(R0, R1, flow), F.update_matrices(R0, R1, flow), "update_matrices")


def test_update_matrices_border_weights_alone(oracle):
    """Zero flow, R1 = R0 = 1 in every channel: M channel 0 is s^2 (1 + 1/4) with s the border scale of the
    pixel, so the weights themselves (not only their products with data) are compared; out-of-image rows and columns
    (the last ones) included."""
    h, w = 13, 16
    R = np.ones((h, w, 5), np.float32)
    flow = np.zeros((h, w, 2), np.float32)
    got = oracle.update_matrices(R, R, flow)
    _check(got, F.update_matrices(R, R, flow), "update_matrices ones")
    s = F.border_scale(w, h)
    inner = np.ones((h, w), bool)
    inner[-1, :] = inner[:, -1] = False   # the last row / column take the out-of-image branch
    assert np.allclose(got[..., 0][inner], (s * s * 1.25)[inner], rtol=1e-6)


@pytest.mark.parametrize("shape", SHAPES + [(31, 45)], ids=_ids(SHAPES + [(31, 45)]))
def test_blur_solve_every_window(oracle, shape):
    """Windows 2..31 (even ones included: cv2 divides a (2m+1)^2 box by winsize^2) on frames smaller than the window."""
    h, w = shape
    R0, R1, flow = _stage_inputs(shape[0] * 100 + shape[1] + 7, h, w)
    M = oracle.update_matrices(R0, R1, flow)
    for ws in range(2, 32):
        got, _ = oracle.update_flow_blur(R0, R1, flow, M, ws, False)
        _check(got, F.blur_solve(M, ws), f"blur_solve winsize={ws}")


def test_blur_solve_positive_definite_field(oracle):
    """A field where G is well conditioned and h varies: the solve's output is of order 1, so the bound is tight."""
    h, w = 37, 29
    rng = np.random.default_rng(4)
    M = rng.random((h, w, 5)).astype(np.float32) + np.float32([3, 0, 3, 0, 0])
    R = np.zeros((h, w, 5), np.float32)
    for ws in (2, 3, 8, 15, 31):
        got, _ = oracle.update_flow_blur(R, R, np.zeros((h, w, 2), np.float32), M, ws, False)
        _check(got, F.blur_solve(M, ws), f"blur_solve winsize={ws}")


# ---------------------------------------------------------------- the whole pipeline, known answers
PARAMS = {"A": (0.5, 3, 15, 3, 5, 1.2, 0), "B": (0.6, 3, 3, 3, 10, 1.05, 0), "C": (0.6, 3, 4, 2, 1, 1.05, 0)}


@pytest.mark.parametrize("name", PARAMS)
@pytest.mark.parametrize("value", [0, 1, 128, 255])
def test_constant_frames_give_zero_flow(oracle, name, value):
    """Identical constant frames: every expansion coefficient but the constant one is zero or cancels in R0 - R1, so
    the flow is exactly zero everywhere, the out-of-image column and row included."""
    a = np.full((70, 90), value, np.uint8)
    assert not oracle.farneback(a, a, *PARAMS[name]).any()


def translated_pair(seed, h, w, dx, dy):
    """A smooth 8-bit texture and the same texture moved by (dx, dy) whole pixels (next(x + dx, y + dy) = prev(x, y))."""
    from test_float_reference import smooth_field
    big = np.rint(smooth_field(seed, h + 2 * 12, w + 2 * 12, 0.0, 255.0, np.float64)).astype(np.uint8)
    prev = big[12:12 + h, 12:12 + w]
    nxt = big[12 - dy:12 - dy + h, 12 - dx:12 - dx + w]
    return np.ascontiguousarray(prev), np.ascontiguousarray(nxt)


# (dx, dy) per parameter set; a 5-pixel move is beyond what B's 3-pixel window and C's levels follow at this size.
# Allowed interior error: mean 0.01 px, 95th percentile 0.02 px (the oracle measures at most 0.003 / 0.008 here).
SHIFTS = [(1, 0), (0, -2), (3, 2), (-5, 4)]
CASES = [(n, s) for s in SHIFTS for n in PARAMS if s != (-5, 4) or n == "A"]


@pytest.mark.parametrize("name,shift", CASES, ids=[f"{n}-{s[0]}_{s[1]}" for n, s in CASES])
def test_integer_translation_is_recovered(oracle, name, shift):
    dx, dy = shift
    prev, nxt = translated_pair(21, 120, 160, dx, dy)
    flow = oracle.farneback(prev, nxt, *PARAMS[name])
    err = np.hypot(flow[..., 0] - dx, flow[..., 1] - dy)[24:-24, 24:-24]
    assert err.mean() < 0.01 and np.percentile(err, 95) < 0.02, (err.mean(), np.percentile(err, 95))
