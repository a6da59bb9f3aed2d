"""CPU: a float-input Farneback reference assembled from the oracle's exposed stages, proven on 8-bit input.

cv2's ``FarnebackOpticalFlowImpl::calc`` converts every frame to float32 first; after that the pipeline is depth-blind.
The oracle only takes uint8 frames, so the float reference here is

* ``blur_f32``: a NumPy float32 replica of the oracle's ``gaussian_blur_f32`` in the default (unfused) variant --
  row taps, then column taps, BORDER_REFLECT_101, every product and sum rounded to float32 (the oracle is compiled with
  ``-ffp-contract=off``, so this is the same arithmetic);
* ``pyr_level_f32`` = ``blur_f32`` + ``oracle.resize_linear``;
* ``farneback_f32``: the oracle's coarse-to-fine driver step for step from ``polyexp``, ``update_matrices``,
  ``update_flow_blur`` and ``resize_linear``.

Both are pinned here to ``oracle.pyr_level`` / ``oracle.farneback`` bit for bit on 8-bit frames; the GPU tests
(tests/test_float_input_gpu.py) then compare the float path of the library against them."""
import numpy as np
import pytest

from nsof.farneback import PARAMS_A, PARAMS_B, PARAMS_C

PARAM_SETS = {"A": PARAMS_A, "B": PARAMS_B, "C": PARAMS_C}
# pyramid geometries beyond A/B/C: the pyr_scale / levels ranges the parameter fuzz of the GPU suite draws from
FUZZ_SCALES = (0.3, 0.4, 0.45, 0.55, 0.7, 0.8)


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def blur_f32(src, ksize, sigma, kernel):
    """GaussianBlur of a float32 image exactly as the oracle's default variant computes it (see module doc)."""
    src = np.ascontiguousarray(src, np.float32)
    if ksize == 1:
        return src.copy()
    k = np.asarray(kernel(ksize, sigma), np.float32)
    h, w = src.shape
    r = ksize // 2
    kc = k[r:]   # kc[j] = centre + j
    cols = _reflect101(np.arange(-r, w + r), w)

    def S(j):   # S[ix[j]] for every x: column x + j, reflected
        return src[:, cols[r + j:r + j + w]]

    if ksize == 3:
        t = (S(-1) + S(1)) * kc[1] + S(0) * kc[0]
    elif ksize == 5:
        t = (S(-2) + S(2)) * kc[2] + ((S(-1) + S(1)) * kc[1] + S(0) * kc[0])
    else:
        t = k[0] * S(-r)
        for j in range(1, ksize):
            t = k[j] * S(j - r) + t
    t = t.astype(np.float32, copy=False)
    rows = _reflect101(np.arange(-r, h + r), h)

    def T(j):
        return t[rows[r + j:r + j + h], :]

    if ksize == 3:
        d = (T(-1) + T(1)) * kc[1] + T(0) * kc[0]
    else:
        d = kc[0] * T(0)
        for j in range(1, r + 1):
            d = kc[j] * (T(j) + T(-j)) + d
    return d.astype(np.float32, copy=False)


def pyr_level_f32(O, img, pyr_scale, k):
    """Pyramid level k of a float32 frame: blur of the full-resolution frame, then resize(INTER_LINEAR)."""
    h, w = img.shape
    wk, hk, ks, sg = O.level_geometry(w, h, pyr_scale, k)
    return O.resize_linear(blur_f32(img, ks, sg, O.gaussian_kernel), wk, hk)


def farneback_f32(O, prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags=0):
    """The oracle's nsof_ref_farneback_u8 driver, stage for stage, on float32 frames."""
    assert flags == 0
    prev = np.asarray(prev, np.float32)
    nxt = np.asarray(nxt, np.float32)
    h, w = prev.shape
    L = O.effective_levels(w, h, pyr_scale, levels)
    flow = None
    for k in range(L, -1, -1):
        wk, hk, _, _ = O.level_geometry(w, h, pyr_scale, k)
        if flow is None:
            flow = np.zeros((hk, wk, 2), np.float32)
        else:
            flow = O.resize_linear(flow, wk, hk) * np.float32(1.0 / pyr_scale)
        R0 = O.polyexp(pyr_level_f32(O, prev, pyr_scale, k), poly_n, poly_sigma)
        R1 = O.polyexp(pyr_level_f32(O, nxt, pyr_scale, k), poly_n, poly_sigma)
        M = O.update_matrices(R0, R1, flow)
        for i in range(iterations):
            flow, M = O.update_flow_blur(R0, R1, flow, M, winsize, i < iterations - 1)
    return flow


def smooth_field(seed, h, w, lo, hi, dtype=np.float32):
    """A smooth random field in [lo, hi] (blurred noise plus a gradient), the kind of frame the flow tracks."""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal((h // 4 + 3, w // 4 + 3))
    n = np.kron(n, np.ones((4, 4)))[:h, :w]
    for _ in range(3):
        n = (np.roll(n, 1, 0) + np.roll(n, -1, 0) + np.roll(n, 1, 1) + np.roll(n, -1, 1) + 4 * n) / 8
    yy, xx = np.mgrid[0:h, 0:w]
    n = n + 0.3 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    n = (n - n.min()) / max(n.max() - n.min(), 1e-12)
    return (lo + (hi - lo) * n).astype(dtype)


def shifted_pair(seed, h, w, lo, hi, dx=1.5, dy=-0.75):
    """(prev, next) float32 with next = prev shifted by (dx, dy) (bilinear), both smooth in [lo, hi]."""
    big = smooth_field(seed, h + 8, w + 8, lo, hi, np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    x0, y0 = xx + 4 - dx, yy + 4 - dy
    xi, yi = np.floor(x0).astype(int), np.floor(y0).astype(int)
    fx, fy = x0 - xi, y0 - yi
    nxt = ((1 - fx) * (1 - fy) * big[yi, xi] + fx * (1 - fy) * big[yi, xi + 1] + (1 - fx) * fy * big[yi + 1, xi]
           + fx * fy * big[yi + 1, xi + 1])
    return big[4:4 + h, 4:4 + w].astype(np.float32), nxt.astype(np.float32)


def _u8_pair(seed, h, w):
    from nsof import synth
    return synth.make_pair(seed, h, w)


def _level_cases():
    cases = []
    for name, p in PARAM_SETS.items():
        for k in range(0, p.levels + 1):
            cases.append((name, p.pyr_scale, k))
    for s in FUZZ_SCALES:
        for k in range(1, 6):
            cases.append(("fuzz", s, k))
    return cases


@pytest.mark.parametrize("name,pyr_scale,k", _level_cases())
def test_blur_resize_is_oracle_pyr_level(oracle, name, pyr_scale, k):
    O = oracle
    img, _ = _u8_pair(11, 301, 389)
    h, w = img.shape
    if k > O.effective_levels(w, h, pyr_scale, 8):
        pytest.skip("level beyond the pyramid of this shape")
    ref = O.pyr_level(img, pyr_scale, k)
    got = pyr_level_f32(O, img.astype(np.float32), pyr_scale, k)
    assert got.shape == ref.shape
    assert np.array_equal(got.view(np.int32), ref.view(np.int32)), f"{name} pyr_scale={pyr_scale} level {k}"


def test_blur_kernel_sizes_covered(oracle):
    """The level cases above reach every kernel-size form of the blur: 3, 5 (small-filter taps) and larger ones."""
    sizes = {oracle.level_geometry(389, 301, s, k)[2] for _, s, k in _level_cases()
             if k <= oracle.effective_levels(389, 301, s, 8)}
    assert {3, 5} <= sizes and max(sizes) >= 19, sorted(sizes)


@pytest.mark.parametrize("name,shape", [("A", (96, 128)), ("B", (77, 101)), ("C", (120, 64)), ("A", (33, 50))])
def test_float_driver_is_oracle_farneback(oracle, name, shape):
    O = oracle
    p = PARAM_SETS[name]
    prev, nxt = _u8_pair(5, *shape)
    args = [getattr(p, f) for f in ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags")]
    ref = O.farneback(prev, nxt, *args)
    got = farneback_f32(O, prev.astype(np.float32), nxt.astype(np.float32), *args)
    assert np.array_equal(got.view(np.int32), ref.view(np.int32))


def test_float_entries_are_exported_and_bound(nsof_lib):
    """The float entry points and the float accumulator surface are in the library and in the binding table."""
    from nsof import _lib
    lib = _lib.load()
    for name in ("nsof_farneback_f32", "nsof_farneback_f32_batch_dev", "nsof_farneback_f32_sequence_dev",
                 "nsof_stage_pyr_level_f32", "nsof_accum_surface_f32_dev"):
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    from nsof.accumulator import Accumulator
    assert callable(getattr(Accumulator, "surface_f32", None))
