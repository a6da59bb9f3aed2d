"""Event denoising on the device: the background-activity filter (``nsof_events_denoise_mark_dev`` / ``_compact_dev``,
csrc/events_denoise.hip), the spatiotemporal correlation filter of the event-camera tool chains, in
integers throughout.  It takes the ``(x, y, p, t)`` stream ``events_from_frames_dev`` emits, where it lies in HBM, and returns
the kept events, the keep mask and the per-pixel state with which a later call continues the run.
"""
import ctypes as C

import numpy as np

from . import _lib
from .errors import NsofValueError
from .events import _STREAM, _empty_stream, _whole

NEVER = -(1 << 63)             # the state of a pixel no event has been seen at
DENOISE_KEYS = ("dt_us", "radius", "min_support", "same_polarity", "include_self", "last")


def _flag(who, name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise NsofValueError(f"{who}: {name} = {v!r} is neither True nor False", _lib.NSOF_EINVAL)
    return int(v)


def _bounds_arg(who, bounds, n):
    if bounds is None:
        return None
    b = np.asarray(bounds)
    if b.dtype.kind not in "iu" or b.ndim != 1:
        raise NsofValueError(f"{who}: bounds must be whole numbers in one dimension (got {b.dtype} {b.shape})", _lib.NSOF_ESHAPE)
    if len(b) and (int(b.min()) < 0 or int(b.max()) > n or (np.diff(b.astype(np.int64)) < 0).any()):
        raise NsofValueError(f"{who}: bounds must not decrease and lie in [0, {n}], the stream's length (got {int(b.min())} .. "
                             f"{int(b.max())})", _lib.NSOF_EINVAL)
    return np.ascontiguousarray(b, np.int64)


def filter_args(who, sensor_hw, dt_us, radius=1, min_support=1, same_polarity=False, include_self=False, last=None):
    """The filter's own arguments checked on the host -> ``(h, w, dt_us, radius, min_support, same_polarity, include_self)`` as
    the library takes them; ``last`` is checked against the sensor and ``same_polarity`` (its device: by the caller, with the
    stream's).  ``events_denoise_dev`` refuses through this, and so does ``video_to_flow_sequence(denoise=...)`` before the
    generator runs."""
    import torch
    if not isinstance(sensor_hw, (tuple, list)) or len(sensor_hw) != 2:
        raise NsofValueError(f"{who}: sensor_hw = {sensor_hw!r}; (H, W) expected", _lib.NSOF_ESHAPE)
    h, w = (_whole(who, "sensor_hw", v) for v in sensor_hw)
    if not (1 <= h <= 32767 and 1 <= w <= 32767):
        raise NsofValueError(f"{who}: sensor_hw = {h}x{w} is beyond the int16 coordinates of an event (1 .. 32767)", _lib.NSOF_ESHAPE)
    dt_us = _whole(who, "dt_us", dt_us)
    if not 0 <= dt_us < 1 << 31:
        raise NsofValueError(f"{who}: dt_us = {dt_us} must be in [0, 2^31)", _lib.NSOF_EINVAL)
    radius = _whole(who, "radius", radius)
    if radius not in (1, 2):
        raise NsofValueError(f"{who}: radius = {radius}; 1 or 2 expected", _lib.NSOF_EINVAL)
    min_support = _whole(who, "min_support", min_support)
    if not 1 <= min_support <= (2 * radius + 1) ** 2:
        raise NsofValueError(f"{who}: min_support = {min_support} must be in [1, {(2 * radius + 1) ** 2}], the pixels of the window",
                             _lib.NSOF_EINVAL)
    same_polarity, include_self = _flag(who, "same_polarity", same_polarity), _flag(who, "include_self", include_self)
    c = 2 if same_polarity else 1
    if last is not None and (not isinstance(last, torch.Tensor) or last.dtype != torch.int64 or tuple(last.shape) != (c, h, w) or
                             not last.is_contiguous()):
        raise NsofValueError(f"{who}: last must be a contiguous int64 tensor [{c}][{h}][{w}] ({c} plane{'s' if c == 2 else ''} "
                             f"with same_polarity={bool(same_polarity)}; got {getattr(last, 'dtype', type(last))} "
                             f"{tuple(getattr(last, 'shape', ()))})", _lib.NSOF_ESHAPE)
    return h, w, dt_us, radius, min_support, same_polarity, include_self


def events_denoise_dev(x, y, p, t, sensor_hw, dt_us, *, radius=1, min_support=1, same_polarity=False, include_self=False,
                       bounds=None, last=None, ctx=None):
    """The background-activity filter on an event stream in HBM.  ``x``, ``y`` (int16), ``p`` (int8), ``t`` (int64): contiguous
    CUDA tensors of ``N`` events (``N < 2^31``) on a ``sensor_hw = (H, W)`` sensor, ``t`` non-decreasing, any int64 -- what
    ``events_from_frames_dev`` returns.  ``last`` is the state, int64 ``[C][H][W]``, ``C = 2`` with ``same_polarity`` (plane 0
    for ``p > 0``, plane 1 otherwise), else 1: the time of the latest event seen at a pixel, ``NEVER`` (the smallest int64)
    for none; ``None`` starts every pixel there.  In stream order, event ``i`` at pixel ``q`` is kept iff at least
    ``min_support`` (``[1, (2 * radius + 1)^2]``) pixels ``m`` of the square of ``radius`` (1 or 2) around ``q``, clipped to the
    sensor and without ``q`` itself unless ``include_self``, have ``last[m] >= max(t_i - dt_us, NEVER + 1)``; then
    ``last[q] = t_i``, kept or not, so a decision depends on the input stream alone.  ``dt_us``: whole, ``[0, 2^31)``.

    Returns a dict: the kept events ``x, y, p, t`` (CUDA, input order), ``keep`` (uint8 CUDA ``[N]``), ``n_kept``, ``bounds``
    (host int64: for ``bounds`` -- non-decreasing, in ``[0, N]``, e.g. the generator's ``frame_bounds`` -- the kept events
    before each, the bounds of the kept stream; ``None`` without) and ``last`` (int64 CUDA ``[C][H][W]``) for the next chunk:
    events ``[0, k)`` and then ``[k, N)`` with the first call's ``last`` give the mask, the kept stream and the final ``last``
    of the one-shot call, bit for bit, for any ``k``.  Every refusal of the arguments raises ``NsofValueError`` before any
    device work; a coordinate outside the sensor or a decreasing ``t`` is found on the device and raises it (``NSOF_EINVAL``)
    from the mark pass, before anything is written.

    Streams: as for ``events_from_frames_dev``.  The call waits for the device once before it starts
    (``torch.cuda.synchronize``: the stream and ``last`` are torch's work), the mark entry waits for the context's stream to
    return ``n_kept``, the compact pass is then queued and the call returns: until ``ctx.synchronize()`` the caller must
    neither read the result elsewhere nor free or overwrite the inputs.  The call owns no temporary that the queued kernels
    read.  ``N = 0`` returns empty tensors and the incoming (or all-``NEVER``) ``last``."""
    import torch

    from .context import default_context, dev_ptr
    who = "events_denoise_dev"
    for (name, dtype), v in zip(_STREAM, (x, y, p, t)):
        if not isinstance(v, torch.Tensor) or v.dtype != getattr(torch, dtype):
            raise NsofValueError(f"{who}: {name} must be an {dtype} tensor (got {getattr(v, 'dtype', type(v))})", _lib.NSOF_EINVAL)
        if v.dim() != 1 or v.shape != x.shape or not v.is_contiguous():
            raise NsofValueError(f"{who}: {name} must be contiguous, one-dimensional and as long as x (got {tuple(v.shape)}, x "
                                 f"{tuple(x.shape)})", _lib.NSOF_ESHAPE)
    n = int(x.shape[0])
    if n >= 1 << 31:
        raise NsofValueError(f"{who}: {n} events, 2^31 or more", _lib.NSOF_EUNSUPPORTED)
    h, w, dt_us, radius, min_support, same_polarity, include_self = filter_args(who, sensor_hw, dt_us, radius, min_support,
                                                                              same_polarity, include_self, last)
    b_in = _bounds_arg(who, bounds, n)
    c = 2 if same_polarity else 1
    if not x.is_cuda or any(v.device != x.device for v in (y, p, t)) or (last is not None and last.device != x.device):
        raise NsofValueError(f"{who}: x, y, p, t (and last) must be CUDA tensors on one device", _lib.NSOF_EINVAL)

    ctx = ctx or default_context()
    dev = x.device
    lib = ctx._lib
    keep = torch.empty(n, dtype=torch.uint8, device=dev)   # fresh allocations: no pending work of torch's to wait for
    n_b = 0 if b_in is None else len(b_in)
    b_out = np.zeros(n_b, np.int64)
    n_kept = C.c_int64(0)
    stream = (ctx.ptr, dev_ptr(x), dev_ptr(y), dev_ptr(p), dev_ptr(t), n, h, w)
    torch.cuda.synchronize(dev)   # the stream and last are torch's work; the library reads them on the context's stream
    ctx.check(lib.nsof_events_denoise_mark_dev(*stream, dt_us, radius, min_support, same_polarity, include_self, dev_ptr(last),
                                               None if b_in is None else b_in.ctypes.data_as(C.c_void_p), n_b, dev_ptr(keep),
                                               C.byref(n_kept), b_out.ctypes.data_as(C.c_void_p)), who)
    total = int(n_kept.value)
    out = _empty_stream(total, dev)
    last_out = torch.empty((c, h, w), dtype=torch.int64, device=dev)
    ctx.check(lib.nsof_events_denoise_compact_dev(*stream, same_polarity, dev_ptr(last), dev_ptr(keep), total,
                                                  *(dev_ptr(out[k]) for k, _ in _STREAM), dev_ptr(last_out)), who)
    return dict(out, keep=keep, n_kept=total, bounds=None if b_in is None else b_out, last=last_out)
