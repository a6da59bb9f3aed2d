"""Event streams from frame sequences, generated on the device (``nsof_events_from_frames_count_dev`` / ``_emit_dev``,
csrc/events_from_frames.hip): a per-pixel level-crossing event generator, the contrast-threshold
model of an event camera, in integers throughout.  A video that is already in HBM becomes an ``(x, y, p, t)`` stream in
the ``/CD/events`` schema, which every event entry of the package takes.

``events_from_frames_dev`` is the generator, ``events_from_video_dev`` the same behind ``gray_u8_dev``;
``render_box_frames`` draws the frames of the reference's ``generate_synthetic_events`` (event_mem_sim.py:109-158), of
which the generator with a threshold of one grey level (any in (1/2, 1]), ``ref=None`` and ``timestamps="frame"`` gives
exactly the events.
"""
import ctypes as C

import numpy as np

from . import _lib
from .accumulator import DT
from .errors import NsofValueError

LEVELS_PER_GREY = 256          # the units of the default (linear) response table: lut[i] = 256 * i
LUT_MAX = 1 << 30
_TIMESTAMPS = {"frame": _lib.EVENTS_T_FRAME, "linear": _lib.EVENTS_T_LINEAR}


def render_box_frames(H=240, W=320, box_h=50, box_w=50, speed_pps=300, duration_s=1.5):  # noqa: N803
    """The binary frames ``generate_synthetic_events`` (event_mem_sim.py:109-158) differences, and their times: a box of
    ones moving left to right over zeros, one frame every ``DT`` seconds.  Returns ``(frames uint8 [n][H][W], times_us
    int64 [n])``.  Host helper (test input)."""
    t_step_us = int(DT * 1_000_000)
    times = np.arange(0, int(duration_s * 1_000_000), t_step_us, dtype=np.int64)
    frames = np.zeros((len(times), H, W), np.uint8)
    y0 = (H - box_h) // 2
    r0, r1 = max(y0, 0), max(min(y0 + box_h, H), 0)
    for k, t_us in enumerate(times):
        start = int((int(t_us) / 1_000_000) * speed_pps)
        end = start + box_w
        if start < W and end > 0:
            frames[k, r0:r1, max(0, start):min(W, end)] = 1
    return frames, times


def linear_response():
    """The default response table: ``256 * i``, 1/256 grey level units."""
    return np.arange(256, dtype=np.int32) * LEVELS_PER_GREY


def log_response(eps=1.0):
    """A logarithmic response table with the range of the linear one (grey 0 maps to 0, grey 255 to ``256 * 255``):
    ``lut[i] = round(256 * 255 * (ln(i + eps) - ln(eps)) / (ln(255 + eps) - ln(eps)))``.  Built on the host."""
    i = np.arange(256, dtype=np.float64)
    v = (np.log(i + eps) - np.log(eps)) / (np.log(255.0 + eps) - np.log(eps))
    return np.rint(LEVELS_PER_GREY * 255 * v).astype(np.int32)


def _whole(who, name, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise NsofValueError(f"{who}: {name} = {v!r} is not a whole number", _lib.NSOF_EINVAL)
    return int(v)


def _threshold_units(who, name, v):
    """A threshold in grey levels as table units: round(256 * v), which must be >= 1."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise NsofValueError(f"{who}: {name} = {v!r} is not a finite number", _lib.NSOF_EINVAL)
    c = int(round(LEVELS_PER_GREY * float(v)))
    if c < 1 or c > 0x7fffffff:
        raise NsofValueError(f"{who}: {name} = {v!r} grey levels is {c} table units; 1 .. 2^31 - 1 expected", _lib.NSOF_EINVAL)
    return c


def _times_arg(who, n, times_us, frame_us):
    if (times_us is None) == (frame_us is None):
        raise NsofValueError(f"{who}: give either times_us or frame_us" + (", not both" if times_us is not None else ""),
                             _lib.NSOF_EINVAL)
    if frame_us is not None:
        step = _whole(who, "frame_us", frame_us)
        if step < 1 or step >= 1 << 31:
            raise NsofValueError(f"{who}: frame_us = {step} must be in [1, 2^31)", _lib.NSOF_EINVAL)
        return np.arange(n, dtype=np.int64) * step
    t = np.asarray(times_us)
    if t.dtype.kind not in "iu" or t.ndim != 1 or len(t) != n:
        raise NsofValueError(f"{who}: times_us must be {n} whole numbers, one per frame (got {t.dtype} {t.shape})", _lib.NSOF_ESHAPE)
    t = np.ascontiguousarray(t, np.int64)
    gaps = np.diff(t)
    if n > 1 and (gaps.min() < 1 or gaps.max() >= 1 << 31):
        k = int(np.argmax((gaps < 1) | (gaps >= 1 << 31)))
        raise NsofValueError(f"{who}: times_us[{k + 1}] = {int(t[k + 1])} after {int(t[k])}: the times must increase strictly, by "
                             "less than 2^31", _lib.NSOF_EINVAL)
    return t


def _response_arg(who, response):
    if response is None:
        return linear_response()
    lut = np.asarray(response)
    if lut.dtype.kind not in "iu" or lut.shape != (256,):
        raise NsofValueError(f"{who}: response must be 256 whole numbers (got {lut.dtype} {lut.shape})", _lib.NSOF_ESHAPE)
    if lut.min() < 0 or lut.max() > LUT_MAX:
        raise NsofValueError(f"{who}: response entries must lie in [0, 2^30] (got {int(lut.min())} .. {int(lut.max())})", _lib.NSOF_EINVAL)
    return np.ascontiguousarray(lut, np.int32)


def _threshold_plane(who, threshold_maps, h, w):
    """``threshold_maps`` (grey levels, ``[H][W][2]``: c_on, c_off per pixel) as a host int32 plane of table units."""
    import torch
    m = threshold_maps.detach().cpu().numpy() if isinstance(threshold_maps, torch.Tensor) else np.asarray(threshold_maps)
    if m.dtype.kind not in "iuf" or m.shape != (h, w, 2):
        raise NsofValueError(f"{who}: threshold_maps must be numbers [{h}][{w}][2] (got {m.dtype} {m.shape})", _lib.NSOF_ESHAPE)
    m = m.astype(np.float64)
    if not np.isfinite(m).all():
        raise NsofValueError(f"{who}: threshold_maps holds a value that is not finite", _lib.NSOF_EINVAL)
    units = np.rint(LEVELS_PER_GREY * m)
    if units.min() < 1 or units.max() > 0x7fffffff:
        y, x, s = (int(v) for v in np.argwhere((units < 1) | (units > 0x7fffffff))[0])
        raise NsofValueError(f"{who}: threshold_maps[{y}][{x}][{s}] = {m[y, x, s]!r} grey levels is {int(units[y, x, s])} table units; "
                             "1 .. 2^31 - 1 expected", _lib.NSOF_EINVAL)
    return np.ascontiguousarray(units.astype(np.int32))


def _polarity_arg(who, name, v):
    v = _whole(who, name, v)
    if not -128 <= v <= 127:
        raise NsofValueError(f"{who}: {name} = {v} does not fit an int8", _lib.NSOF_EINVAL)
    return v


def events_from_frames_dev(frames, times_us=None, *, frame_us=None, threshold=10.0, threshold_off=None, threshold_maps=None,
                           response=None, ref=None, timestamps="linear", p_on=1, p_off=-1, ctx=None):
    """A frame sequence in HBM as an event stream in HBM (``nsof_events_from_frames_*_dev``).  ``frames``: uint8 CUDA
    tensor ``[n][H][W]``, frame and row strides free, pixels of a row dense.  Times in microseconds: ``times_us`` (``n``
    whole numbers, strictly increasing by less than 2^31) or ``frame_us`` (frame ``k`` at ``k * frame_us``).  With
    ``L[k] = response[F[k]]`` (``response``: 256 whole numbers in [0, 2^30]; ``None``: ``256 * i``, so that the units are
    1/256 grey level; ``log_response()`` gives a logarithmic one) every pixel keeps a reference level ``r`` and per frame
    emits ``(L - r) // c_on`` ON events if that is at least one, else ``(r - L) // c_off`` OFF events, one per threshold
    crossed, and moves ``r`` by as many thresholds.  ``threshold`` / ``threshold_off`` (``None``: the same) are in grey
    levels, ``c = round(256 * threshold) >= 1``; ``threshold_maps`` (``[H][W][2]`` grey levels, array or tensor, checked on
    the host) replaces both per pixel.  ``ref``: ``None`` starts ``r`` from zeros (the reference generator's black
    ``prev_frame``), ``"first"`` from the first frame's levels (frame 0 emits nothing), an int32 CUDA tensor ``[H][W]`` --
    the ``ref`` of a previous result -- continues that run: over ``frames[0:k+1]`` and then ``frames[k:n]`` the two calls
    give the stream and the final ``ref`` of the one-shot call, bit for bit.  ``timestamps="frame"`` stamps the events of
    frame ``k`` with its time; ``"linear"`` takes the level to move linearly between frames ``k-1`` and ``k`` and stamps a
    crossing of level ``l`` ``T[k-1] + (|l - L[k-1]| * (T[k] - T[k-1])) // |L[k] - L[k-1]|`` (frame 0 of a call: ``T[0]``).
    Frames come in order and within a frame the events ascend by (t, ON before OFF, y, x, crossing).

    Returns a dict: CUDA tensors ``x``, ``y`` (int16), ``p`` (int8: ``p_on`` / ``p_off``; ``p_off=0`` gives the ``/CD/events``
    convention), ``t`` (int64), the host int64 array ``frame_bounds`` ``[n + 1]`` (the events of frame ``k`` are
    ``[frame_bounds[k], frame_bounds[k+1])``) and ``ref`` (int32 CUDA ``[H][W]``) for the next chunk.  Every refusal of the
    arguments raises ``NsofValueError`` before any device work; a stream of 2^31 or more events raises it from the count
    pass, before anything is emitted.

    Streams: the library works on the context's stream, not torch's.  The call waits for the device once before it starts
    (``torch.cuda.synchronize``: the frames and ``ref`` are torch's work) and the count entry waits for the context's stream
    to return the bounds; the emit pass is then queued and the call returns.  Until ``ctx.synchronize()`` the caller must
    neither read the result elsewhere nor free or overwrite ``frames`` and ``ref`` (torch's caching allocator reuses a freed
    block on torch's stream at once).  The one temporary of the call's own that the queued kernels read, the uploaded
    ``threshold_maps`` plane, is covered here: with ``threshold_maps`` the call ends in ``ctx.synchronize()``."""
    import torch

    from .context import default_context, dev_ptr
    who = "events_from_frames_dev"
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8:
        raise NsofValueError(f"{who}: frames must be a uint8 tensor (got {getattr(frames, 'dtype', type(frames))})", _lib.NSOF_EINVAL)
    if frames.dim() != 3 or min(frames.shape) < 1 or (frames.shape[2] > 1 and frames.stride(2) != 1):
        raise NsofValueError(f"{who}: frames must be [n][H][W] with dense rows (got {tuple(frames.shape)}, strides "
                             f"{tuple(frames.stride())})", _lib.NSOF_ESHAPE)
    n, h, w = (int(v) for v in frames.shape)
    if h > 32767 or w > 32767:
        raise NsofValueError(f"{who}: {h}x{w} frames are beyond the int16 coordinates of an event", _lib.NSOF_ESHAPE)
    times = _times_arg(who, n, times_us, frame_us)
    lut = _response_arg(who, response)
    c_on = _threshold_units(who, "threshold", threshold)
    c_off = c_on if threshold_off is None else _threshold_units(who, "threshold_off", threshold_off)
    plane = None if threshold_maps is None else _threshold_plane(who, threshold_maps, h, w)
    if timestamps not in _TIMESTAMPS:
        raise NsofValueError(f"{who}: timestamps = {timestamps!r}; 'frame' or 'linear' expected", _lib.NSOF_EINVAL)
    p_on, p_off = _polarity_arg(who, "p_on", p_on), _polarity_arg(who, "p_off", p_off)
    if ref is None or (isinstance(ref, str) and ref == "first"):
        ref_mode, ref_in = (_lib.EVENTS_REF_ZERO if ref is None else _lib.EVENTS_REF_FIRST), None
    elif isinstance(ref, torch.Tensor):
        if ref.dtype != torch.int32 or tuple(ref.shape) != (h, w) or not ref.is_contiguous():
            raise NsofValueError(f"{who}: ref must be a contiguous int32 tensor [{h}][{w}] (got {ref.dtype} {tuple(ref.shape)})",
                                 _lib.NSOF_ESHAPE)
        ref_mode, ref_in = _lib.EVENTS_REF_GIVEN, ref
    else:
        raise NsofValueError(f"{who}: ref = {ref!r}; None, 'first' or the ref of a previous result expected", _lib.NSOF_EINVAL)
    if not frames.is_cuda or (ref_in is not None and ref_in.device != frames.device):
        raise NsofValueError(f"{who}: frames (and ref) must be CUDA tensors on one device", _lib.NSOF_EINVAL)

    ctx = ctx or default_context()
    dev = frames.device
    d_plane = None if plane is None else torch.from_numpy(plane).to(dev)
    bounds = np.empty(n + 1, np.int64)
    common = (dev_ptr(frames), int(frames.stride(1)), int(frames.stride(0)), n, h, w, times.ctypes.data_as(C.c_void_p),
              lut.ctypes.data_as(C.c_void_p), c_on, c_off, dev_ptr(d_plane), dev_ptr(ref_in), ref_mode,
              bounds.ctypes.data_as(C.c_void_p))
    torch.cuda.synchronize(dev)   # the frames, ref and the plane's upload are torch's work; the library reads them on the context's stream
    try:
        ctx.check(ctx._lib.nsof_events_from_frames_count_dev(ctx.ptr, *common), who)
        total = int(bounds[n])
        x, y = (torch.empty(total, dtype=torch.int16, device=dev) for _ in range(2))
        p = torch.empty(total, dtype=torch.int8, device=dev)
        t = torch.empty(total, dtype=torch.int64, device=dev)
        ref_out = torch.empty((h, w), dtype=torch.int32, device=dev)   # fresh allocations: no pending work of torch's to wait for
        ctx.check(ctx._lib.nsof_events_from_frames_emit_dev(ctx.ptr, *common, _TIMESTAMPS[timestamps], p_on, p_off, total, dev_ptr(x),
                                                            dev_ptr(y), dev_ptr(p), dev_ptr(t), dev_ptr(ref_out)), who)
    finally:
        if d_plane is not None:
            # the queued kernels read the uploaded plane, and torch's allocator hands a freed block to the next allocation
            # on torch's stream at once: the plane may go only when the context's stream has drained
            ctx.synchronize()
    return dict(x=x, y=y, p=p, t=t, frame_bounds=bounds, ref=ref_out)


def events_from_video_dev(frames_bgr, times_us=None, *, code="BGR2GRAY", ctx=None, **kwargs):
    """``events_from_frames_dev`` of a colour video in HBM: ``frames_bgr`` uint8 CUDA tensor ``[n][H][W][3]`` goes through
    ``gray_u8_dev`` (cv2's fixed-point ``cvtColor``; ``code``: ``"BGR2GRAY"`` or ``"RGB2GRAY"``) frame by frame into one grey
    stack, which the generator reads.  Every other argument as there.  The grey stack is this call's own and the queued emit
    pass reads it, so the call ends in ``ctx.synchronize()``: the result is complete on return."""
    import torch

    from .context import default_context
    from .predict import gray_u8_dev
    who = "events_from_video_dev"
    if not isinstance(frames_bgr, torch.Tensor) or frames_bgr.dtype != torch.uint8 or frames_bgr.dim() != 4 or \
            frames_bgr.shape[3] != 3 or min(frames_bgr.shape) < 1:
        raise NsofValueError(f"{who}: frames must be a uint8 tensor [n][H][W][3]", _lib.NSOF_ESHAPE)
    if code not in ("RGB2GRAY", "BGR2GRAY"):
        raise NsofValueError(f"{who}: code must be RGB2GRAY or BGR2GRAY", _lib.NSOF_EINVAL)
    if not frames_bgr.is_cuda:
        raise NsofValueError(f"{who}: frames must be a CUDA tensor", _lib.NSOF_EINVAL)
    ctx = ctx or default_context()
    n, h, w = (int(v) for v in frames_bgr.shape[:3])
    gray = torch.empty((n, h, w), dtype=torch.uint8, device=frames_bgr.device)
    torch.cuda.synchronize(frames_bgr.device)
    for k in range(n):
        gray_u8_dev(frames_bgr[k], gray[k], code, ctx=ctx)
    ctx.synchronize()
    try:
        return events_from_frames_dev(gray, times_us, ctx=ctx, **kwargs)
    finally:
        ctx.synchronize()   # the queued emit pass walks the grey stack, which is freed on return
