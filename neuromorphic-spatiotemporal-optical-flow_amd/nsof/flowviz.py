"""Middlebury colour coding of a flow field: host-side mirror of the reference's ``flow_viz`` module
(/root/reference/flow_viz.py:20-135 -- ``make_colorwheel``, ``flow_uv_to_colors``, ``flow_to_image``), which the
scripts use to write their flow PNGs (``viz``, optical_flow_seg.py:106-113).  SURVEY.md section 8f row 4.

The colour wheel is the published one of Baker et al. (ICCV 2007): 55 hues in six segments RY/YG/GC/CB/BM/MR of
15/6/4/11/13/6 steps.  Hue = direction, saturation = magnitude / max magnitude; vectors longer than the
normaliser are dimmed to 75 %.  Plain NumPy on the host (a presentation step, not on the hot path); float64
like the reference, which feeds it the float64 canvas of ``opticalFlow3D``.

``flow_to_image_dev`` is the same coding on the device (``nsof_flow_to_image_dev``, csrc/flowviz_kernels.hip) for
batches of float32 flows in HBM, the prediction experiment's ``viz`` of every pair; ``save_viz`` writes its images.
"""
import numpy as np

_SEGMENTS = (("RY", 15), ("YG", 6), ("GC", 4), ("CB", 11), ("BM", 13), ("MR", 6))


def make_colorwheel():
    """[55, 3] float64 RGB wheel.  Each segment ramps one channel up or down while another sits at 255."""
    n = sum(k for _, k in _SEGMENTS)
    wheel = np.zeros((n, 3))
    # (channel held at 255, channel ramped, ramp direction) per segment
    plan = ((0, 1, +1), (1, 0, -1), (1, 2, +1), (2, 1, -1), (2, 0, +1), (0, 2, -1))
    at = 0
    for (_, k), (hold, ramp, sign) in zip(_SEGMENTS, plan):
        step = np.floor(255 * np.arange(k) / k)
        wheel[at:at + k, hold] = 255
        wheel[at:at + k, ramp] = step if sign > 0 else 255 - step
        at += k
    return wheel


def flow_uv_to_colors(u, v, convert_to_bgr=False):
    """u, v already divided by the normaliser.  Returns uint8 [H, W, 3]."""
    u = np.asarray(u)
    v = np.asarray(v)
    wheel = make_colorwheel()
    n = wheel.shape[0]
    rad = np.sqrt(np.square(u) + np.square(v))
    pos = (np.arctan2(-v, -u) / np.pi + 1) / 2 * (n - 1)
    lo = np.floor(pos).astype(np.int32)
    hi = lo + 1
    hi[hi == n] = 0
    frac = pos - lo
    small = rad <= 1
    img = np.zeros(u.shape + (3,), np.uint8)
    for c in range(3):
        col = (1 - frac) * (wheel[lo, c] / 255.0) + frac * (wheel[hi, c] / 255.0)
        col = np.where(small, 1 - rad * (1 - col), col * 0.75)
        img[..., 2 - c if convert_to_bgr else c] = np.floor(255 * col)
    return img


def flow_to_image(flow_uv, clip_flow=None, convert_to_bgr=False, max_flow=None):
    """flow_uv [H, W, 2] -> uint8 [H, W, 3].  Normalised by the largest magnitude (+1e-5) unless max_flow is given."""
    flow_uv = np.asarray(flow_uv)
    if flow_uv.ndim != 3 or flow_uv.shape[2] != 2:
        raise ValueError("input flow must have shape [H,W,2]")
    if clip_flow is not None:
        flow_uv = np.clip(flow_uv, 0, clip_flow)
    u, v = flow_uv[..., 0], flow_uv[..., 1]
    top = np.max(np.sqrt(np.square(u) + np.square(v))) if max_flow is None else max_flow
    return flow_uv_to_colors(u / (top + 1e-5), v / (top + 1e-5), convert_to_bgr)


def viz(flo, imgname):
    """``viz`` of the scripts (optical_flow_seg.py:11-19): colour-code the flow and save it with the channels in
    B,G,R order, as the reference does (it hands ``flo[:, :, [2, 1, 0]]`` to PIL).  Needs Pillow."""
    from PIL import Image
    img = flow_to_image(flo)[:, :, [2, 1, 0]]
    Image.fromarray(np.ascontiguousarray(img)).save(imgname)


def flow_to_image_dev(flows, out=None, *, clip_flow=None, max_flow=None, convert_to_bgr=False, sign=1, norms=None,
                      ctx=None):
    """``flow_to_image`` of ``sign * flows`` on the device (``nsof_flow_to_image_dev``).  ``flows``: float32 CUDA tensor
    [H][W][2] or [n][H][W][2], (u, v) interleaved; rows and items may be strided (a crop of a larger canvas).  Each
    flow is normalised by its own largest magnitude + 1e-5, or by ``max_flow`` + 1e-5 when given.  Returns ``out``,
    uint8 [n][H][W][3] ([H][W][3] for one flow; allocated when None, else any view with interleaved pixels), equal to
    ``flow_to_image(sign * flow, clip_flow, convert_to_bgr, max_flow)`` of each float32 flow, with atan2 rounded
    once from float64 (NumPy's float32 arctan2 is off by an ulp now and then, so its output differs on about one pixel
    in a million, by one level).  Non-finite flows, which the NumPy coding cannot colour, are defined: pixels with a NaN
    magnitude ((inf, NaN) among them) do not enter the largest magnitude, an infinite magnitude (an infinite component,
    or a finite one whose float32 square overflows) makes the divisor +inf, a pixel whose normalised u or v is NaN is
    (0, 0, 0) (a colour no finite flow gets), and an infinite normalised component is coloured like any pixel outside
    the unit circle.
    ``norms`` (float32 CUDA tensor [n]) receives each flow's float32 divisor.
    Asynchronous on the context's stream: ``ctx.synchronize()`` before reading ``out`` elsewhere."""
    import torch

    from . import _lib
    from .context import default_context, dev_ptr
    from .errors import NsofValueError
    if not isinstance(flows, torch.Tensor) or not flows.is_cuda:
        raise NsofValueError("flow_to_image_dev: flows must be a CUDA tensor", _lib.NSOF_EINVAL)
    if flows.dtype != torch.float32:
        raise NsofValueError(f"flow_to_image_dev: float32 flows expected (got {flows.dtype})", _lib.NSOF_EINVAL)
    single = flows.dim() == 3
    f = flows.unsqueeze(0) if single else flows
    if f.dim() != 4 or f.shape[3] != 2 or f.stride(3) != 1 or f.stride(2) != 2 or min(f.shape) < 1:
        raise NsofValueError(f"flow_to_image_dev: [H][W][2] or [n][H][W][2] flows with contiguous rows expected (got "
                             f"{tuple(flows.shape)})", _lib.NSOF_ESHAPE)
    for name, val in (("clip_flow", clip_flow), ("max_flow", max_flow)):
        if val is not None and not float(val) >= 0:
            raise NsofValueError(f"flow_to_image_dev: {name} must be >= 0 (got {val})", _lib.NSOF_EINVAL)
    if sign not in (1, -1):
        raise NsofValueError("flow_to_image_dev: sign must be +1 or -1", _lib.NSOF_EINVAL)
    n, h, w = (int(v) for v in f.shape[:3])
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=flows.device)
        torch.cuda.synchronize(flows.device)
        if single:
            out = out[0]
    o = out.unsqueeze(0) if single and isinstance(out, torch.Tensor) and out.dim() == 3 else out
    if not isinstance(o, torch.Tensor) or not o.is_cuda or o.dtype != torch.uint8 or tuple(o.shape) != (n, h, w, 3) \
            or o.stride(3) != 1 or o.stride(2) != 3:
        raise NsofValueError(f"flow_to_image_dev: out must be a uint8 CUDA tensor {(n, h, w, 3)} with interleaved "
                             "pixels", _lib.NSOF_ESHAPE)
    if norms is not None and (not isinstance(norms, torch.Tensor) or not norms.is_cuda or norms.dtype != torch.float32
                              or tuple(norms.shape) != (n,) or not norms.is_contiguous()):
        raise NsofValueError(f"flow_to_image_dev: norms must be a contiguous float32 CUDA tensor [{n}]", _lib.NSOF_ESHAPE)
    ctx = ctx or default_context()
    rc = ctx._lib.nsof_flow_to_image_dev(
        ctx.ptr, n, dev_ptr(f), int(f.stride(1)), int(f.stride(0)), w, h, int(sign),
        -1.0 if clip_flow is None else float(clip_flow), -1.0 if max_flow is None else float(max_flow),
        int(bool(convert_to_bgr)), dev_ptr(o), int(o.stride(1)), int(o.stride(0)), dev_ptr(norms))
    ctx.check(rc, "flow_to_image_dev")
    return out


def save_viz(images, paths):
    """Write a batch of device images (uint8 [n][H][W][3], e.g. ``viz_mem`` of ``prediction_sequence_dev``, whose
    channels are already in the B,G,R order ``viz`` hands to PIL) as one PNG per path, after ONE device-to-host copy.
    Each file holds the pixels ``viz(-flow, path)`` writes for that pair's flow.  Needs Pillow."""
    from PIL import Image
    paths = list(paths)
    if images.dim() != 4 or images.shape[3] != 3 or int(images.shape[0]) != len(paths):
        raise ValueError(f"save_viz: {len(paths)} paths for images of shape {tuple(images.shape)}")
    host = images.cpu().numpy()
    for img, path in zip(host, paths):
        Image.fromarray(np.ascontiguousarray(img)).save(path)
