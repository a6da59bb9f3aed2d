"""CPU: the definition ``nsof_flow_to_image_dev`` (csrc/flowviz_kernels.hip) computes, restated in NumPy, reproduces the
reference's own ``flow_viz.py`` goldens; the Python entry refuses host and float64 input before the library is called;
the C entry is exported and bound.

``cr_flow_to_image`` is ``nsof.flow_to_image`` on float32 input as NumPy 2 promotes it, with one change: atan2 is
``float32(atan2(float64(y), float64(x)))``, rounded once, where NumPy's float32 arctan2 is a few ulp off on some inputs
and depends on the host's SIMD dispatch.  The GPU tests compare the device against it byte for byte.
"""
import numpy as np
import pytest

from conftest import golden_path


def cr_flow_to_image(flow, clip_flow=None, convert_to_bgr=False, max_flow=None):
    """[H][W][2] float32 -> uint8 [H][W][3], step by step in the precision NumPy 2 gives each step on float32 input."""
    from nsof import flowviz
    flow = np.asarray(flow)
    assert flow.dtype == np.float32 and flow.ndim == 3 and flow.shape[2] == 2
    if clip_flow is not None:
        flow = np.clip(flow, 0, clip_flow)                     # float32; -0.0 stays -0.0
    u, v = flow[..., 0], flow[..., 1]
    if max_flow is None:
        d = np.max(np.sqrt(np.square(u) + np.square(v))) + np.float32(1e-5)
    else:
        d = np.float32(float(max_flow) + 1e-5)
    d = np.float32(d)
    u, v = u / d, v / d                                       # float32, correctly rounded
    wheel = flowviz.make_colorwheel()
    n = wheel.shape[0]
    rad = np.sqrt(np.square(u) + np.square(v))
    a = np.arctan2(-v.astype(np.float64), -u.astype(np.float64)).astype(np.float32)
    pos = (a / np.float32(np.pi) + np.float32(1)) / np.float32(2) * np.float32(n - 1)
    assert pos.dtype == np.float32
    lo = np.floor(pos).astype(np.int32)
    hi = lo + 1
    hi[hi == n] = 0
    frac = pos - lo                                           # float64: float32 minus int32 promotes
    assert frac.dtype == np.float64
    small = rad <= 1
    img = np.zeros(u.shape + (3,), np.uint8)
    for c in range(3):
        col = (1 - frac) * (wheel[lo, c] / 255.0) + frac * (wheel[hi, c] / 255.0)
        col = np.where(small, 1 - rad.astype(np.float64) * (1 - col), col * 0.75)
        img[..., 2 - c if convert_to_bgr else c] = np.floor(255 * col)
    return img


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
