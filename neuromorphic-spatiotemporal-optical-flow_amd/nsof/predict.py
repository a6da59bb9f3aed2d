"""Frame prediction by flow warp + SSIM: host-side mirror of the prediction task of
/root/reference/optical_flow_prediction.py (``task_results`` :255-353, baseline warp :581-591,
``calculateIntegralError`` :113-115) and of the cv2 / scikit-image calls inside it.  SURVEY.md section 8f row 2.

    flow_map = (grid + flow).astype(np.float32)
    new_frame[y0:y1, x0:x1, c] = cv2.remap(next_frame[:, :, c], flow_map[..., 0], flow_map[..., 1],
                                           cv2.INTER_LINEAR, borderMode=cv2.BORDER_REPLICATE)
    ssim = structural_similarity(true[:, :, 2], new_frame[:, :, 2], data_range=255.0)

All per-pixel work runs in libnsof.so (csrc/warp_kernels.hip): the map is formed inside the warp kernel from the flow,
the three channels are warped together, the SSIM statistics are exact integer window sums reduced in a fixed order.
"""
import time

import numpy as np

from . import _lib
from .context import default_context, dev_ptr
from .errors import NsofValueError

INTER_LINEAR = 1                         # cv2.INTER_LINEAR
BORDER_CONSTANT, BORDER_REPLICATE = 0, 1  # cv2.BORDER_*


def gray_u8_dev(d_frame, d_gray, code="RGB2GRAY", *, ctx=None):
    """``cv2.cvtColor(frame, COLOR_RGB2GRAY | COLOR_BGR2GRAY)`` on DEVICE memory: ``d_frame`` uint8 [H][W][3] torch CUDA
    tensor (rows may be strided), ``d_gray`` uint8 [H][W].  Same bytes as ``nsof.gating.frame_to_gray``; asynchronous on
    the context's stream -- decoded frames need not visit the host before the flow call."""
    ctx = ctx or default_context()
    if code not in ("RGB2GRAY", "BGR2GRAY"):
        raise NsofValueError("gray_u8_dev: code must be RGB2GRAY or BGR2GRAY", _lib.NSOF_EINVAL)
    h, w = int(d_frame.shape[0]), int(d_frame.shape[1])
    if tuple(d_frame.shape) != (h, w, 3) or tuple(d_gray.shape) != (h, w) or d_frame.stride(2) != 1 or d_frame.stride(1) != 3 \
            or d_gray.stride(1) != 1:
        raise NsofValueError("gray_u8_dev: uint8 [H][W][3] interleaved frame and [H][W] output expected", _lib.NSOF_ESHAPE)
    rc = ctx._lib.nsof_gray_u8_dev(ctx.ptr, dev_ptr(d_frame), int(d_frame.stride(0)), w, h, 1 if code == "BGR2GRAY" else 0,
                                   dev_ptr(d_gray), int(d_gray.stride(0)))
    ctx.check(rc, "gray_u8_dev")
    return d_gray


def remap(src, map1, map2, interpolation=INTER_LINEAR, dst=None, borderMode=BORDER_CONSTANT, borderValue=0,  # noqa: N803
          *, ctx=None):
    """``cv2.remap`` for uint8 images (1 or 3 channels), two float32 maps and INTER_LINEAR."""
    import torch
    ctx = ctx or default_context()
    if interpolation != INTER_LINEAR:
        raise NsofValueError("remap: only INTER_LINEAR is provided", _lib.NSOF_EUNSUPPORTED)
    src = np.asarray(src)
    if src.dtype != np.uint8 or src.ndim not in (2, 3):
        raise NsofValueError("remap: uint8 image expected", _lib.NSOF_EINVAL)
    map1 = np.ascontiguousarray(map1, np.float32)
    map2 = np.ascontiguousarray(map2, np.float32)
    if map1.ndim != 2 or map1.shape != map2.shape:
        raise NsofValueError("remap: map1 and map2 must be 2-D float32 arrays of one shape", _lib.NSOF_ESHAPE)
    if isinstance(borderValue, (tuple, list)):
        borderValue = borderValue[0]  # noqa: N806
    cn = 1 if src.ndim == 2 else src.shape[2]
    sh, sw = src.shape[:2]
    dh, dw = map1.shape
    dev = torch.device("cuda", ctx.device)
    d_src = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
    d_mx, d_my = torch.from_numpy(map1).to(dev), torch.from_numpy(map2).to(dev)
    d_dst = torch.empty((dh, dw) if src.ndim == 2 else (dh, dw, cn), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    rc = ctx._lib.nsof_remap_linear_u8_dev(ctx.ptr, dev_ptr(d_src), sw * cn, sw, sh, cn, dev_ptr(d_mx), dw,
                                           dev_ptr(d_my), dw, dw, dh, int(borderMode), int(borderValue),
                                           dev_ptr(d_dst), dw * cn)
    ctx.check(rc, "remap")
    ctx.synchronize()
    out = d_dst.cpu().numpy()
    if dst is not None:
        dst[...] = out
        return dst
    return out


def predict_region(next_frame, flow, rect, out=None, sign=-1, borderMode=BORDER_REPLICATE, *, ctx=None):  # noqa: N803
    """Warp ``next_frame`` inside ``rect = (x0, y0, x1, y1)`` with ``sign * flow`` (``flow`` = the frame-sized flow
    canvas, un-negated Farneback output for ``sign=-1``); the rest of ``out`` (default: a copy of the frame,
    prediction.py:263) is left as it is."""
    ctx = ctx or default_context()
    frame = np.asarray(next_frame)
    if frame.dtype != np.uint8 or frame.ndim not in (2, 3) or (frame.ndim == 3 and frame.strides[2] != 1):
        raise NsofValueError("predict_region: uint8 frame expected", _lib.NSOF_EINVAL)
    if frame.strides[1] != (1 if frame.ndim == 2 else frame.shape[2]):
        frame = np.ascontiguousarray(frame)
    h, w = frame.shape[:2]
    cn = 1 if frame.ndim == 2 else frame.shape[2]
    x0, y0, x1, y1 = (int(v) for v in rect)
    if out is None:
        out = frame.copy()
    if x1 <= x0 or y1 <= y0:
        return out
    crop = np.asarray(flow)[y0:y1, x0:x1]
    if crop.dtype != np.float32 or crop.strides[2] != 4 or crop.strides[1] != 8:
        crop = np.ascontiguousarray(crop, np.float32)     # float64 canvases hold float32 values
    rc = ctx._lib.nsof_predict_warp_u8(ctx.ptr, frame.ctypes.data, frame.strides[0], w, h, cn, crop.ctypes.data,
                                       crop.strides[0], int(sign), x0, y0, x1, y1, int(borderMode), out.ctypes.data,
                                       out.strides[0])
    ctx.check(rc, "predict_region")
    return out


def predict_region_dev(d_frame, d_flow, d_out, height, width, rect, channels=3, sign=-1, borderMode=BORDER_REPLICATE,  # noqa: N803
                       *, ctx=None):
    """Device-resident variant (torch tensors or raw addresses, dense layouts); asynchronous."""
    ctx = ctx or default_context()
    x0, y0, x1, y1 = (int(v) for v in rect)
    rc = ctx._lib.nsof_predict_warp_u8_dev(ctx.ptr, dev_ptr(d_frame), width * channels, width, height, channels,
                                           dev_ptr(d_flow), 2 * width, int(sign), x0, y0, x1, y1, int(borderMode),
                                           dev_ptr(d_out), width * channels)
    ctx.check(rc, "predict_region_dev")


def task_results(prev_frame, next_frame, flow, num_labels, regions_info, EST_FLAG=2, MERGE_FLAG=False, padding=20,  # noqa: N803
                 sign=1, times=None, *, ctx=None, comb_times=None, borderMode=BORDER_REPLICATE):  # noqa: N803
    """optical_flow_prediction.py:255-353.  ``flow`` is the canvas the caller already negated (:545), hence
    ``sign=1`` here; pass the raw ``opticalFlow3D`` canvas with ``sign=-1`` to skip that host pass.  ``times`` /
    ``comb_times`` (lists) receive the task's time and the time up to its box list, as the script's
    ``mem_task_times`` / ``mem_combination_times``; ``borderMode`` is the remap's (the script's full-frame baseline,
    :584-586, is this task on the box (0, 0, w, h) with BORDER_CONSTANT)."""
    t0 = time.time()
    h, w = prev_frame.shape[:2]
    new_frame = np.array(next_frame, copy=True)
    if num_labels > 1:
        if EST_FLAG == 1 and MERGE_FLAG:
            boxes = [(max(0, min(r[0] for r in regions_info) - padding), max(0, min(r[1] for r in regions_info) - padding),
                      min(w, max(r[2] for r in regions_info) + padding), min(h, max(r[3] for r in regions_info) + padding))]
        elif EST_FLAG == 1:
            boxes = list(regions_info)
        else:
            boxes = [tuple(regions_info)]
        if comb_times is not None:
            comb_times.append(time.time() - t0)
        for box in boxes:   # later boxes see the original frame, like the reference (it always warps next_frame)
            predict_region(next_frame, flow, box, out=new_frame, sign=sign, borderMode=borderMode, ctx=ctx)
    elif comb_times is not None:
        comb_times.append(time.time() - t0)
    if times is not None:
        times.append(time.time() - t0)
    return new_frame


def structural_similarity(im1, im2, data_range=255.0, *, ctx=None):
    """``skimage.metrics.structural_similarity(im1, im2, data_range=...)`` with its defaults, for 2-D uint8 views."""
    ctx = ctx or default_context()
    a, b = np.asarray(im1), np.asarray(im2)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.ndim != 2 or a.shape != b.shape:
        raise NsofValueError("structural_similarity: two uint8 2-D images of one shape expected", _lib.NSOF_ESHAPE)
    if min(a.shape) < 7:
        raise NsofValueError("win_size exceeds image extent", _lib.NSOF_ESHAPE)
    if a.strides[1] < 1 or b.strides[1] < 1:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    import ctypes as C
    out = C.c_double()
    rc = ctx._lib.nsof_ssim_u8(ctx.ptr, a.ctypes.data, a.strides[0], a.strides[1], b.ctypes.data, b.strides[0],
                               b.strides[1], a.shape[1], a.shape[0], float(data_range), C.byref(out))
    ctx.check(rc, "structural_similarity")
    return out.value


def calculateIntegralError(prediction, true, *, ctx=None):  # noqa: N802
    """optical_flow_prediction.py:113-115: SSIM of channel 2 (red of a BGR frame)."""
    return structural_similarity(np.asarray(true)[:, :, 2], np.asarray(prediction)[:, :, 2], data_range=255.0, ctx=ctx)


def _u8_frames(t, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NsofValueError(f"{what}: a CUDA tensor expected", _lib.NSOF_EINVAL)
    if t.dtype != torch.uint8:
        raise NsofValueError(f"{what}: uint8 expected (got {t.dtype})", _lib.NSOF_EINVAL)


def predict_sequence_dev(frames_bgr, flows, out=None, *, counts=None, rects=None, gate_frame=0, merge_padding=None,
                         border_mode=BORDER_REPLICATE, sign=-1, ctx=None):
    """The prediction step of every pair of a sequence in one launch (``nsof_predict_sequence_u8_dev``): pair k warps
    frame k+1 of ``frames_bgr`` (uint8 CUDA tensor [n][H][W][3], pixels interleaved, row / frame strides free) with
    ``sign * flows[k]`` (float32 CUDA tensor [n_pairs][H][W][2], contiguous; n >= n_pairs + 1) into ``out[k]`` (uint8
    [n_pairs][H][W][3], contiguous; allocated when None).  Region of pair k: the rectangles of row ``k + gate_frame`` of
    the device table ``counts`` / ``rects`` (``gating.roi_from_surface_dev``, the table the ROI flow call consumed) --
    their union (``merge_padding=None``: FLAG 1 separate, FLAG 2) or their bounding box padded by ``merge_padding`` and
    clipped (FLAG 1 merged, the script's PADDING 20) -- with the frame copied elsewhere; without a table the whole frame
    (the full-frame baseline: pass ``border_mode=BORDER_CONSTANT``).  Each ``out[k]`` equals ``task_results`` of that
    pair bit for bit.  The table's counts must not exceed ``rects.shape[1]`` (``gating.rects_to_host`` checks it).
    Asynchronous on the context's stream."""
    import torch
    ctx = ctx or default_context()
    _u8_frames(frames_bgr, "predict_sequence_dev")
    if not isinstance(flows, torch.Tensor) or not flows.is_cuda or flows.dtype != torch.float32:
        raise NsofValueError("predict_sequence_dev: flows must be a float32 CUDA tensor", _lib.NSOF_EINVAL)
    if frames_bgr.dim() != 4 or frames_bgr.shape[3] != 3 or frames_bgr.stride(3) != 1 or frames_bgr.stride(2) != 3:
        raise NsofValueError("predict_sequence_dev: frames must be [n][H][W][3] with interleaved pixels", _lib.NSOF_ESHAPE)
    n, h, w = (int(v) for v in frames_bgr.shape[:3])
    n_pairs = int(flows.shape[0]) if flows.dim() == 4 else 0
    if tuple(flows.shape) != (n_pairs, h, w, 2) or not flows.is_contiguous() or n_pairs < 1 or n < n_pairs + 1:
        raise NsofValueError(f"predict_sequence_dev: flows {tuple(flows.shape)} do not fit {n} frames of {h}x{w} "
                             "(contiguous [n_pairs][H][W][2], n_pairs <= n - 1)", _lib.NSOF_ESHAPE)
    if (counts is None) != (rects is None):
        raise NsofValueError("predict_sequence_dev: pass counts and rects together", _lib.NSOF_EINVAL)
    n_maps = max_rects = 0
    if counts is not None:
        if counts.dtype != torch.int32 or rects.dtype != torch.int32 or not counts.is_contiguous() or \
                not rects.is_contiguous() or rects.dim() != 3 or rects.shape[2] != 4 or counts.shape != rects.shape[:1]:
            raise NsofValueError("predict_sequence_dev: counts int32 [n_maps] and rects int32 [n_maps][max_rects][4] "
                                 "(contiguous) expected", _lib.NSOF_ESHAPE)
        n_maps, max_rects = int(rects.shape[0]), int(rects.shape[1])
    if out is None:
        out = torch.empty((n_pairs, h, w, 3), dtype=torch.uint8, device=frames_bgr.device)
        torch.cuda.synchronize(frames_bgr.device)
    else:
        _u8_frames(out, "predict_sequence_dev")
        if tuple(out.shape) != (n_pairs, h, w, 3) or not out.is_contiguous():
            raise NsofValueError("predict_sequence_dev: out must be a contiguous uint8 [n_pairs][H][W][3] tensor",
                                 _lib.NSOF_ESHAPE)
    rc = ctx._lib.nsof_predict_sequence_u8_dev(
        ctx.ptr, n_pairs, dev_ptr(frames_bgr), int(frames_bgr.stride(1)), int(frames_bgr.stride(0)), w, h, dev_ptr(flows),
        int(sign), dev_ptr(counts), dev_ptr(rects), n_maps, max_rects, int(gate_frame),
        -1 if merge_padding is None else int(merge_padding), int(border_mode), dev_ptr(out))
    ctx.check(rc, "predict_sequence_dev")
    return out


def ssim_batch_dev(a, b, channel=2, out=None, *, ctx=None):
    """``structural_similarity(b[i][..., channel], a[i][..., channel], data_range=255)`` of every pair i at once
    (``nsof_ssim_u8_batch_dev``): ``a`` / ``b`` uint8 CUDA tensors [n][H][W][C] (``channel`` selects one interleaved
    channel; default 2 = ``calculateIntegralError``) or [n][H][W]; results in ``out`` (float64 CUDA tensor [n],
    allocated when None), each equal to the single-pair ``nsof_ssim_u8_dev`` exactly.  Asynchronous."""
    import torch
    ctx = ctx or default_context()
    _u8_frames(a, "ssim_batch_dev")
    _u8_frames(b, "ssim_batch_dev")
    if a.shape != b.shape or a.dim() not in (3, 4) or a.shape[0] < 1:
        raise NsofValueError(f"ssim_batch_dev: two [n][H][W][C] or [n][H][W] tensors of one shape expected (got "
                             f"{tuple(a.shape)}, {tuple(b.shape)})", _lib.NSOF_ESHAPE)
    n, h, w = (int(v) for v in a.shape[:3])
    if a.dim() == 4:
        if not 0 <= int(channel) < a.shape[3] or a.stride(3) != 1 or b.stride(3) != 1:
            raise NsofValueError("ssim_batch_dev: channel out of range or channels not interleaved", _lib.NSOF_ESHAPE)
        off = int(channel)
    else:
        off = 0
    if min(h, w) < 7:
        raise NsofValueError("ssim_batch_dev: win_size 7 exceeds the image extent", _lib.NSOF_ESHAPE)
    if out is None:
        out = torch.empty((n,), dtype=torch.float64, device=a.device)
        torch.cuda.synchronize(a.device)
    elif out.dtype != torch.float64 or tuple(out.shape) != (n,) or not out.is_contiguous() or not out.is_cuda:
        raise NsofValueError("ssim_batch_dev: out must be a contiguous float64 CUDA tensor [n]", _lib.NSOF_ESHAPE)
    rc = ctx._lib.nsof_ssim_u8_batch_dev(
        ctx.ptr, n, dev_ptr(b) + off, int(b.stride(1)), int(b.stride(0)), int(b.stride(2)), dev_ptr(a) + off,
        int(a.stride(1)), int(a.stride(0)), int(a.stride(2)), w, h, 255.0, dev_ptr(out))
    ctx.check(rc, "ssim_batch_dev")
    return out
