"""CPU: the definition ``nsof_flow_to_image_dev`` (csrc/flowviz_kernels.hip) computes, restated in NumPy, reproduces the
reference's own ``flow_viz.py`` goldens; the Python entry refuses host and float64 input before the library is called;
the C entry is exported and bound.

``cr_flow_to_image`` is ``nsof.flow_to_image`` on float32 input as NumPy 2 promotes it, with one change: atan2 is
``float32(atan2(float64(y), float64(x)))``, rounded once, where NumPy's float32 arctan2 is a few ulp off on some inputs
and depends on the host's SIMD dispatch.  The GPU tests compare the device against it byte for byte.

``cr_flow_to_image_nonfinite`` is the same definition with the kernel header's answers for NaN and infinite flows, where
the NumPy coding has none; it is pinned here to hand-derived colours and is what tests/test_heads_nonfinite_gpu.py
compares the device with.
"""
import numpy as np
import pytest

from conftest import golden_path


def cr_flow_to_image(flow, clip_flow=None, convert_to_bgr=False, max_flow=None):
    """[H][W][2] float32 -> uint8 [H][W][3], step by step in the precision NumPy 2 gives each step on float32 input."""
    return cr_flow_to_image_nonfinite(flow, clip_flow, convert_to_bgr, max_flow)[0]


def cr_flow_to_image_nonfinite(flow, clip_flow=None, convert_to_bgr=False, max_flow=None):
    """``cr_flow_to_image`` extended to NaN and infinite flows as csrc/flowviz_kernels.hip and ``flow_to_image_dev``
    define them -> (uint8 [H][W][3], the float32 divisor).  On finite flows every step is the NumPy coding's; the three
    additions are: the largest magnitude skips NaN magnitudes (an fmax reduction from 0, so an all-NaN flow has 0 and
    an infinite component +inf); a pixel whose normalised u or v is NaN (a NaN flow, inf / inf) is black; everything
    else, an infinite normalised component included, takes the ordinary steps (atan2 of infinities is finite, rad is
    +inf, so the pixel is outside the unit circle: wheel colour times 0.75)."""
    from nsof import flowviz
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] == 2
    with np.errstate(over="ignore", invalid="ignore"):   # 3e38 squared, inf / inf, inf * 0 in the branch np.where drops
        if clip_flow is not None:
            flow = np.clip(flow, 0, clip_flow)                 # float32; -0.0 stays -0.0, NaN stays NaN, +inf -> clip
            assert flow.dtype == np.float32
        u, v = flow[..., 0], flow[..., 1]
        if max_flow is None:
            mag = np.sqrt(np.square(u) + np.square(v))
            assert mag.dtype == np.float32
            d = np.fmax.reduce(mag, axis=None, initial=np.float32(0)) + np.float32(1e-5)
        else:
            d = np.float32(float(max_flow) + 1e-5)
        d = np.float32(d)
        u, v = u / d, v / d                                   # float32, correctly rounded
        black = np.isnan(u) | np.isnan(v)
        u, v = np.where(black, np.float32(0), u), np.where(black, np.float32(0), v)   # any value the wheel can index
        wheel = flowviz.make_colorwheel()
        n = wheel.shape[0]
        rad = np.sqrt(np.square(u) + np.square(v))
        a = np.arctan2(-v.astype(np.float64), -u.astype(np.float64)).astype(np.float32)
        pos = (a / np.float32(np.pi) + np.float32(1)) / np.float32(2) * np.float32(n - 1)
        assert pos.dtype == np.float32
        lo = np.floor(pos).astype(np.int32)
        hi = lo + 1
        hi[hi == n] = 0
        frac = pos - lo                                       # float64: float32 minus int32 promotes
        assert frac.dtype == np.float64
        small = rad <= 1
        img = np.zeros(u.shape + (3,), np.uint8)
        for c in range(3):
            col = (1 - frac) * (wheel[lo, c] / 255.0) + frac * (wheel[hi, c] / 255.0)
            col = np.where(small, 1 - rad.astype(np.float64) * (1 - col), col * 0.75)
            img[..., 2 - c if convert_to_bgr else c] = np.floor(255 * col)
        img[black] = 0
    return img, d


def golden_cases():
    with np.load(golden_path("flowviz_golden.npz")) as z:
        return {name: {k: z[f"{name}_{k}"] for k in ("flow", "rgb", "bgr", "clip")}
                for name in ("smooth", "noise", "tiny", "zero", "f64")}


def test_cr_reference_reproduces_goldens(nsof_lib):
    for name, g in golden_cases().items():
        if name == "f64":
            continue   # the device entry is float32 only
        assert np.array_equal(cr_flow_to_image(g["flow"]), g["rgb"]), name
        assert np.array_equal(cr_flow_to_image(g["flow"], convert_to_bgr=True), g["bgr"]), name
        assert np.array_equal(cr_flow_to_image(g["flow"], clip_flow=2.5), g["clip"]), name


def test_cr_reference_signed_zeros():
    """atan2(+-0, negative) is +-pi: wheel entry 0 or 54 -- the sign of a zero decides the colour."""
    f = np.array([[[-1.0, 0.0], [-1.0, -0.0]]], np.float32)     # -u = +1 / -v = -0 or +0
    img = cr_flow_to_image(-f)                                  # flow_to_image's own negation inside atan2
    assert not np.array_equal(img[0, 0], img[0, 1])


def _small_field():
    return (np.random.default_rng(5).standard_normal((7, 9, 2)) * 2).astype(np.float32)


def test_nonfinite_reference_equals_the_old_one_on_finite_flows(nsof_lib):
    """The divisor it returns is the NumPy coding's own, np.max(...) + 1e-5 in float32."""
    for name, g in golden_cases().items():
        if name == "f64":
            continue
        u, v = g["flow"][..., 0], g["flow"][..., 1]
        img, d = cr_flow_to_image_nonfinite(g["flow"])
        assert np.array_equal(img, g["rgb"]), name
        assert d.dtype == np.float32 and d == np.max(np.sqrt(np.square(u) + np.square(v))) + np.float32(1e-5), name
        assert cr_flow_to_image_nonfinite(g["flow"], max_flow=3.0)[1] == np.float32(3.0 + 1e-5)


@pytest.mark.parametrize("bad", [(np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan)])
def test_nonfinite_reference_one_nan_pixel(nsof_lib, bad):
    """The NaN pixel is black and takes no part in the divisor: the rest is the finite coding of the field without it."""
    f = _small_field()
    f[3, 4] = (100.0, -100.0)          # were this pixel to count, it would be the largest magnitude
    f[3, 4] = bad
    clean = f.copy()
    clean[3, 4] = (0.0, 0.0)
    assert np.isfinite(clean).all()
    for kw in (dict(), dict(convert_to_bgr=True), dict(clip_flow=2.5), dict(max_flow=3.0)):
        img, d = cr_flow_to_image_nonfinite(f, **kw)
        want, d_clean = cr_flow_to_image_nonfinite(clean, **kw)
        assert np.isfinite(d) and d == d_clean, kw
        assert (img[3, 4] == 0).all(), kw
        other = np.ones(img.shape[:2], bool)
        other[3, 4] = False
        assert np.array_equal(img[other], want[other]), kw
        assert (img[other] != 0).any(-1).all(), kw        # black is no finite flow's colour


def test_nonfinite_reference_inf_beside_nan_is_a_nan_pixel(nsof_lib):
    """(inf, NaN) has the magnitude sqrt(inf + NaN) = NaN: it is skipped like any NaN pixel, so the divisor stays finite."""
    f = _small_field()
    clean = f.copy()
    f[2, 6] = (np.inf, np.nan)
    f[5, 1] = (np.nan, -np.inf)
    clean[2, 6] = clean[5, 1] = (0.0, 0.0)
    img, d = cr_flow_to_image_nonfinite(f)
    want, d_clean = cr_flow_to_image_nonfinite(clean)
    assert np.isfinite(d) and d == d_clean
    assert (img[2, 6] == 0).all() and (img[5, 1] == 0).all()
    img[2, 6] = want[2, 6]
    img[5, 1] = want[5, 1]
    assert np.array_equal(img, want)


@pytest.mark.parametrize("bad", [(np.inf, 0.5), (0.5, -np.inf), (-np.inf, np.inf)])
def test_nonfinite_reference_one_inf_component(nsof_lib, bad):
    """An infinite magnitude makes the divisor +inf: finite / inf = 0 is white (rad 0), inf / inf = NaN is black."""
    f = _small_field()
    f[2, 6] = bad
    f[0, 0] = (np.nan, 1.0)             # a NaN elsewhere changes nothing
    img, d = cr_flow_to_image_nonfinite(f)
    assert np.isposinf(d) and d.dtype == np.float32
    black = np.zeros(img.shape[:2], bool)
    black[2, 6] = black[0, 0] = True
    assert (img[black] == 0).all() and (img[~black] == 255).all()
    f[2, 6] = (3e38, 3e38)              # finite, but its float32 magnitude overflows: the same divisor, and 3e38 / inf = 0
    f[0, 0] = (1.0, 1.0)
    img, d = cr_flow_to_image_nonfinite(f)
    assert np.isposinf(d) and (img == 255).all()


def test_nonfinite_reference_inf_pixel_under_max_flow(nsof_lib):
    """max_flow = 3: the divisor is finite, +-inf stays infinite, atan2 of it is a multiple of pi/2 and rad = +inf is
    outside the unit circle -- floor(255 * (wheel / 255 * 0.75)) of the direction's wheel entry."""
    from nsof import flowviz
    wheel = flowviz.make_colorwheel()
    f = _small_field()
    # (u, v) -> wheel entry: atan2(-v, -u) = -pi, +pi, -0 -> position 0, 54, 27
    cases = {(1, 1): ((np.inf, 0.0), 0), (2, 2): ((np.inf, -0.0), 54), (3, 3): ((-np.inf, 0.0), 27),
             (4, 4): ((np.inf, 2.0), 0), (5, 5): ((-np.inf, 2.0), 27)}      # a finite v over an infinite u: atan2 is +-0 / -pi
    for (y, x), (val, _) in cases.items():
        f[y, x] = val
    f[6, 8] = (np.inf, np.nan)
    f[0, 8] = (-np.inf, np.inf)          # atan2(-inf, +inf) = -pi/4: between two wheel entries
    img, d = cr_flow_to_image_nonfinite(f, max_flow=3.0)
    assert d == np.float32(3.0 + 1e-5)
    assert wheel[0].tolist() == [255, 0, 0] and wheel[54].tolist() == [255, 0, 43] and wheel[27].tolist() == [0, 209, 255]
    hand = {0: [191, 0, 0], 54: [191, 0, 32], 27: [0, 156, 191]}             # floor(0.75 * entry)
    for (y, x), (_, k) in cases.items():
        assert img[y, x].tolist() == hand[k] == np.floor(255 * (wheel[k] / 255.0 * 0.75)).astype(int).tolist(), (y, x)
    assert (img[6, 8] == 0).all()
    assert img[0, 8].any() and img[0, 8].max() == 191
    bgr, _ = cr_flow_to_image_nonfinite(f, max_flow=3.0, convert_to_bgr=True)
    assert np.array_equal(bgr, img[..., ::-1])
    # clip_flow turns +inf into the clip and -inf into +0 (finite pixels), and keeps NaN (black)
    clip, _ = cr_flow_to_image_nonfinite(f, clip_flow=2.5, max_flow=3.0)
    want = np.clip(np.where(np.isnan(f), np.float32(0), f), 0, 2.5).astype(np.float32)
    ref = cr_flow_to_image(want, max_flow=3.0)
    ref[6, 8] = 0
    assert np.array_equal(clip, ref)


def test_flow_to_image_dev_refuses_host_and_float64_input(nsof_lib):
    import torch
    from nsof.errors import NsofValueError
    flow = golden_cases()["noise"]["flow"]
    with pytest.raises(NsofValueError):
        nsof_lib.flow_to_image_dev(flow)
    with pytest.raises(NsofValueError):
        nsof_lib.flow_to_image_dev(torch.from_numpy(flow))
    with pytest.raises(NsofValueError):
        nsof_lib.flow_to_image_dev(torch.from_numpy(golden_cases()["f64"]["flow"]))


def test_flow_to_image_dev_is_exported_and_bound(nsof_lib):
    import ctypes as C
    from nsof import _lib
    lib = _lib.load()
    assert "nsof_flow_to_image_dev" in _lib.SIGNATURES
    fn = lib.nsof_flow_to_image_dev
    assert fn.restype is C.c_int and len(fn.argtypes) == 15
    assert lib.nsof_abi_version() == 3
    # a NULL context is refused before anything else is looked at
    assert fn(None, 1, None, 2, 2, 1, 1, 1, -1.0, -1.0, 0, None, 3, 3, None) == _lib.NSOF_EINVAL
