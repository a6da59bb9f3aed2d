"""Motion-segmentation head: host-side mirror of the reference's ``task_results`` / ``process_flow_region``
(/root/reference/optical_flow_seg.py:253-357; baseline copy :503-537) and of the cv2 calls inside them.
SURVEY.md section 8f row 3.

    mag, ang = cv2.cartToPolar(fx, fy); mask[mag > SEG_TH] = 255
    5 x { cv2.dilate(mask, ellipse 10x10); cv2.erode(mask, ellipse 10x10) }; threshold(1) -> 0/255

Everything per pixel runs in libnsof.so (bit-packed masks, one fused launch for the whole dilate/erode chain;
csrc/segment_kernels.hip).  The hue/value image the reference also builds (:327-343) never reaches its result and
is not computed.
"""
import time

import numpy as np

from . import _lib
from .context import default_context, dev_ptr
from .errors import NsofValueError

MORPH_RECT, MORPH_CROSS, MORPH_ELLIPSE = 0, 1, 2     # cv2.MORPH_*


def getStructuringElement(shape, ksize):  # noqa: N802
    """``cv2.getStructuringElement(shape, (width, height))`` -> uint8 [height][width] of 0/1."""
    kw, kh = int(ksize[0]), int(ksize[1])
    out = np.zeros((max(kh, 0), max(kw, 0)), np.uint8)
    rc = _lib.load().nsof_structuring_element(int(shape), kw, kh, out.ctypes.data)
    if rc:
        raise NsofValueError(f"getStructuringElement({shape}, {ksize}): bad argument", rc)
    return out


def _morph(op, src, kernel, anchor, iterations, ctx):
    import torch
    ctx = ctx or default_context()
    src = np.asarray(src)
    if src.ndim == 3:   # the baseline path pushes a 3-channel copy of the mask through (seg.py:526-533)
        return np.stack([_morph(op, src[..., c], kernel, anchor, iterations, ctx) for c in range(src.shape[2])], -1)
    if src.ndim != 2 or src.dtype != np.uint8:
        raise NsofValueError("dilate/erode: uint8 single-channel mask expected", _lib.NSOF_EINVAL)
    kernel = np.ascontiguousarray(kernel, np.uint8)
    h, w = src.shape
    dev = torch.device("cuda", ctx.device)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    d_dst = torch.empty_like(d_src)
    torch.cuda.synchronize(dev)
    rc = ctx._lib.nsof_morph_binary_u8_dev(ctx.ptr, op, dev_ptr(d_src), w, w, h, kernel.ctypes.data, kernel.shape[1],
                                           kernel.shape[0], int(anchor[0]), int(anchor[1]), int(iterations),
                                           dev_ptr(d_dst), w)
    ctx.check(rc, "dilate" if op else "erode")
    ctx.synchronize()
    return d_dst.cpu().numpy()


def dilate(src, kernel, anchor=(-1, -1), iterations=1, *, ctx=None):
    """``cv2.dilate`` for two-valued uint8 masks (non-zero = set; result 0/255, which is what cv2 returns for the
    0/255 masks the reference feeds it)."""
    return _morph(1, src, kernel, anchor, iterations, ctx)


def erode(src, kernel, anchor=(-1, -1), iterations=1, *, ctx=None):
    """``cv2.erode`` for two-valued uint8 masks."""
    return _morph(0, src, kernel, anchor, iterations, ctx)


def motion_mask(flow, seg_th=1, ksize=10, iterations=5, out=None, *, ctx=None):
    """The whole head on a flow field or a strided crop of one: uint8 [H][W] of 0/255.  float64 canvases (what
    ``opticalFlow3D`` returns) hold float32 values and are narrowed without loss; the sign of the flow is
    irrelevant.  A pixel moves when its float64 magnitude sqrt(u*u + v*v) exceeds ``seg_th``: a NaN component never
    does (not even beside an infinite one: inf + NaN is NaN), an infinite one otherwise exceeds every finite
    threshold, and a finite one whose square overflows float32 (3e38) is compared as the finite float64 it is."""
    ctx = ctx or default_context()
    flow = np.asarray(flow)
    if flow.ndim != 3 or flow.shape[2] != 2:
        raise NsofValueError("flow must have shape [H,W,2]", _lib.NSOF_ESHAPE)
    if flow.dtype != np.float32 or flow.strides[2] != 4 or flow.strides[1] != 8:
        flow = np.ascontiguousarray(flow, np.float32)
    h, w = flow.shape[:2]
    if out is None:
        out = np.empty((h, w), np.uint8)
    if h == 0 or w == 0:
        return out
    rc = ctx._lib.nsof_motion_mask(ctx.ptr, flow.ctypes.data, flow.strides[0], w, h, float(seg_th), int(ksize),
                                   int(iterations), out.ctypes.data, out.strides[0])
    ctx.check(rc, "motion_mask")
    return out


def motion_mask_dev(d_flow, d_mask, height, width, seg_th=1, ksize=10, iterations=5, *, flow_stride=None,
                    mask_stride=None, ctx=None):
    """Device-resident variant (torch tensors or raw addresses); asynchronous on the context's stream."""
    ctx = ctx or default_context()
    rc = ctx._lib.nsof_motion_mask_dev(ctx.ptr, dev_ptr(d_flow), 2 * width if flow_stride is None else flow_stride,
                                       width, height, float(seg_th), int(ksize), int(iterations), dev_ptr(d_mask),
                                       width if mask_stride is None else mask_stride)
    ctx.check(rc, "motion_mask_dev")


def motion_mask_sequence_dev(flows, boxes=None, out=None, seg_th=1, ksize=10, iterations=5, *, ctx=None):
    """The head over the boxes of every pair of a sequence (``nsof_motion_mask_sequence_dev``): ``flows`` float32 CUDA
    tensor [n_pairs][H][W][2] (contiguous), ``boxes`` a list per pair of ``(x0, y0, x1, y1)`` boxes in paste order, or
    None for one whole-frame box per pair (the full-frame baseline).  ``out[k]`` (uint8 [n_pairs][H][W], contiguous;
    allocated when None) is zero except where pair k's boxes lie, and there it is the ``motion_mask`` of the crop of
    the last box that covers the pixel -- ``task_results`` of that pair, bit for bit.  Empty boxes are skipped.
    Asynchronous on the context's stream."""
    import torch
    ctx = ctx or default_context()
    if not isinstance(flows, torch.Tensor) or not flows.is_cuda or flows.dtype != torch.float32:
        raise NsofValueError("motion_mask_sequence_dev: flows must be a float32 CUDA tensor", _lib.NSOF_EINVAL)
    if flows.dim() != 4 or flows.shape[3] != 2 or not flows.is_contiguous() or flows.shape[0] < 1:
        raise NsofValueError(f"motion_mask_sequence_dev: contiguous [n_pairs][H][W][2] flows expected (got "
                             f"{tuple(flows.shape)})", _lib.NSOF_ESHAPE)
    n, h, w = (int(v) for v in flows.shape[:3])
    counts = table = None
    if boxes is not None:
        if len(boxes) != n:
            raise NsofValueError(f"motion_mask_sequence_dev: {len(boxes)} box lists for {n} pairs", _lib.NSOF_ESHAPE)
        counts = np.array([len(b) for b in boxes], np.int32)
        table = np.array([tuple(int(v) for v in r) for b in boxes for r in b], np.int32).reshape(-1, 4)
        table = np.ascontiguousarray(table) if table.size else np.zeros((1, 4), np.int32)
    if out is None:
        out = torch.empty((n, h, w), dtype=torch.uint8, device=flows.device)
        torch.cuda.synchronize(flows.device)
    elif not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.uint8 or \
            tuple(out.shape) != (n, h, w) or not out.is_contiguous():
        raise NsofValueError("motion_mask_sequence_dev: out must be a contiguous uint8 CUDA tensor [n_pairs][H][W]",
                             _lib.NSOF_ESHAPE)
    rc = ctx._lib.nsof_motion_mask_sequence_dev(
        ctx.ptr, n, dev_ptr(flows), w, h, None if counts is None else counts.ctypes.data,
        None if table is None else table.ctypes.data, float(seg_th), int(ksize), int(iterations), dev_ptr(out))
    ctx.check(rc, "motion_mask_sequence_dev")
    return out


def pixel_accuracy_batch_dev(masks, gt_bgr, out=None, *, ctx=None):
    """``calculate_pixel_accuracy(masks[i], (BGR2GRAY(gt_bgr[i]) > 127) * 255)`` of every item at once
    (``nsof_pixel_accuracy_u8_batch_dev``): ``masks`` uint8 CUDA tensor [n][H][W] (contiguous), ``gt_bgr`` uint8 CUDA
    tensor [n][H][W][3] (pixels interleaved, row / frame strides free).  Results in ``out`` (float64 CUDA tensor [n],
    allocated when None), each equal to the host formula exactly.  Asynchronous."""
    import torch
    ctx = ctx or default_context()
    for t, what in ((masks, "masks"), (gt_bgr, "gt_bgr")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8:
            raise NsofValueError(f"pixel_accuracy_batch_dev: {what} must be a uint8 CUDA tensor", _lib.NSOF_EINVAL)
    if masks.dim() != 3 or not masks.is_contiguous() or masks.shape[0] < 1 or gt_bgr.dim() != 4 or \
            tuple(gt_bgr.shape) != tuple(masks.shape) + (3,) or gt_bgr.stride(3) != 1 or gt_bgr.stride(2) != 3:
        raise NsofValueError(f"pixel_accuracy_batch_dev: contiguous masks [n][H][W] and interleaved frames [n][H][W][3] "
                             f"expected (got {tuple(masks.shape)}, {tuple(gt_bgr.shape)})", _lib.NSOF_ESHAPE)
    n, h, w = (int(v) for v in masks.shape)
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=masks.device)
        torch.cuda.synchronize(masks.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != (n,) or \
            not out.is_contiguous() or not out.is_cuda:
        raise NsofValueError("pixel_accuracy_batch_dev: out must be a contiguous float64 CUDA tensor [n]", _lib.NSOF_ESHAPE)
    rc = ctx._lib.nsof_pixel_accuracy_u8_batch_dev(ctx.ptr, n, dev_ptr(masks), dev_ptr(gt_bgr), int(gt_bgr.stride(1)),
                                                   int(gt_bgr.stride(0)), w, h, dev_ptr(out))
    ctx.check(rc, "pixel_accuracy_batch_dev")
    return out


def process_flow_region(mag, ang=None, seg_th=1, *, ctx=None):
    """optical_flow_seg.py:322-357 with the same arguments (``ang`` only feeds the unused hue image)."""
    mask = np.where(np.asarray(mag) > seg_th, np.uint8(255), np.uint8(0))
    k = getStructuringElement(MORPH_ELLIPSE, (10, 10))
    for _ in range(5):
        mask = erode(dilate(mask, k, ctx=ctx), k, ctx=ctx)
    return np.where(mask > 1, np.uint8(255), np.uint8(0))


def task_results(prev_frame, next_frame, flow, num_labels, regions_info, EST_FLAG=2, MERGE_FLAG=False,  # noqa: N803
                 padding=20, seg_th=1, times=None, *, ctx=None):
    """optical_flow_seg.py:253-320: the head on the gated region(s) only, pasted into an all-zero mask.
    ``regions_info`` is what ``opticalFlow3D`` returned (a list of boxes for FLAG 1, one box for FLAG 2)."""
    t0 = time.time()
    h, w = prev_frame.shape[:2]
    motion_binary = np.zeros((h, w), np.uint8)
    if num_labels > 1:
        if EST_FLAG == 1 and MERGE_FLAG:
            boxes = [(max(0, min(r[0] for r in regions_info) - padding), max(0, min(r[1] for r in regions_info) - padding),
                      min(w, max(r[2] for r in regions_info) + padding), min(h, max(r[3] for r in regions_info) + padding))]
        elif EST_FLAG == 1:
            boxes = list(regions_info)
        else:
            boxes = [tuple(regions_info)]
        for x_min, y_min, x_max, y_max in boxes:
            if x_max > x_min and y_max > y_min:
                motion_mask(flow[y_min:y_max, x_min:x_max], seg_th, out=motion_binary[y_min:y_max, x_min:x_max], ctx=ctx)
    if times is not None:
        times.append(time.time() - t0)
    return motion_binary
