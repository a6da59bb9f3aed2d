"""Event streams from frame sequences, generated on the device (``nsof_events_from_frames_count_dev`` / ``_emit_dev``,
csrc/events_from_frames.hip): a per-pixel level-crossing event generator, the contrast-threshold
model of an event camera, in integers throughout.  A video that is already in HBM becomes an ``(x, y, p, t)`` stream in
the ``/CD/events`` schema, which every event entry of the package takes.

``events_from_frames_dev`` is the generator, ``events_from_video_dev`` the same behind ``gray_u8_dev``;
``render_box_frames`` draws the frames of the reference's ``generate_synthetic_events`` (event_mem_sim.py:109-158), of
which the generator with a threshold of one grey level (any in (1/2, 1]), ``ref=None`` and ``timestamps="frame"`` gives
exactly the events.  ``refractory_us`` / ``noise`` / ``t_ok`` / ``first_frame`` add a per-pixel refractory period and
background-activity noise events (``nsof_events_from_frames_sensor_*_dev``); ``events_noise_draw``
gives the noise generator's words on the host.
"""
import ctypes as C
import typing

import numpy as np

from . import _lib
from .accumulator import DT
from .errors import NsofValueError

LEVELS_PER_GREY = 256          # the units of the default (linear) response table: lut[i] = 256 * i
LUT_MAX = 1 << 30
INT64_MAX = (1 << 63) - 1
_TIMESTAMPS = {"frame": _lib.EVENTS_T_FRAME, "linear": _lib.EVENTS_T_LINEAR}
_STREAM = (("x", "int16"), ("y", "int16"), ("p", "int8"), ("t", "int64"))   # the arrays of an event stream and their dtypes


def _empty_stream(total, dev):
    """An output stream of ``total`` events on ``dev``, not yet written: ``{"x": ..., "y": ..., "p": ..., "t": ...}``."""
    import torch
    return {name: torch.empty(total, dtype=getattr(torch, dtype), device=dev) for name, dtype in _STREAM}


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


class _Quantity(typing.NamedTuple):
    """An argument in the caller's units that the library holds in whole units of its own: ``round(v * mul / div)`` (the
    two steps in this order, so that a power of two is exact: one rounding), which must lie in ``[lo, hi]``."""
    mul: float
    div: float
    lo: int
    hi: int
    dtype: type      # of a per-pixel plane
    label: str       # how a message names the argument ``name``
    unit: str        # the caller's unit
    units: str       # the library's
    span: str        # [lo, hi] in words
    shown: object    # a plane's value as its message shows it: NumPy's float64 (thresholds) or a Python float (rates)


_THRESHOLD = _Quantity(float(LEVELS_PER_GREY), 1.0, 1, 0x7fffffff, np.int32, "{}", "grey levels", "table units", "1 .. 2^31 - 1",
                       lambda v: v)
_RATE = _Quantity(4294967296.0, 1e6, 0, (1 << 32) - 1, np.uint32, "noise[{!r}]", "Hz", "units of 2^-32 per microsecond",
                  "0 .. 2^32 - 1", float)


def _units(who, qty, name, v):
    """A number in the caller's units (a threshold in grey levels, a noise rate in Hz) as the library's whole units."""
    label = qty.label.format(name)
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
        raise NsofValueError(f"{who}: {label} = {v!r} is not a finite number", _lib.NSOF_EINVAL)
    u = int(round(float(v) * qty.mul / qty.div))
    if not qty.lo <= u <= qty.hi:
        raise NsofValueError(f"{who}: {label} = {v!r} {qty.unit} is {u} {qty.units}; {qty.span} expected", _lib.NSOF_EINVAL)
    return u


def _units_plane(who, qty, name, maps, h, w):
    """``maps`` (the caller's units, ``[H][W][2]``: ON, OFF per pixel; array or tensor) as a host plane of the library's whole
    units, of ``qty.dtype``."""
    import torch
    label = qty.label.format(name)
    m = maps.detach().cpu().numpy() if isinstance(maps, torch.Tensor) else np.asarray(maps)
    if m.dtype.kind not in "iuf" or m.shape != (h, w, 2):
        raise NsofValueError(f"{who}: {label} must be numbers [{h}][{w}][2] (got {m.dtype} {m.shape})", _lib.NSOF_ESHAPE)
    m = m.astype(np.float64)
    if not np.isfinite(m).all():
        raise NsofValueError(f"{who}: {label} holds a value that is not finite", _lib.NSOF_EINVAL)
    u = np.rint(m * qty.mul / qty.div)
    if u.min() < qty.lo or u.max() > qty.hi:
        y, x, c = (int(v) for v in np.argwhere((u < qty.lo) | (u > qty.hi))[0])
        raise NsofValueError(f"{who}: {label}[{y}][{x}][{c}] = {qty.shown(m[y, x, c])!r} {qty.unit} is {int(u[y, x, c])} {qty.units}; "
                             f"{qty.span} expected", _lib.NSOF_EINVAL)
    return np.ascontiguousarray(u.astype(qty.dtype))


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


NOISE_KEYS = ("seed", "rate_hz", "rate_on_hz", "rate_off_hz", "rate_maps")


def _sensor_args(who, n, h, w, refractory_us, noise, t_ok, first_frame):
    """The four sensor arguments checked on the host -> ``None`` when all are at their defaults (the plain generator),
    else a dict: ``refractory_us``, ``seed``, ``first_frame``, ``rate_on_q``, ``rate_off_q``, ``plane`` (host uint32
    ``[H][W][2]`` or ``None``) and ``t_ok`` (the tensor or ``None``; its device is checked with the frames')."""
    import torch
    refractory_us = _whole(who, "refractory_us", refractory_us)
    if not 0 <= refractory_us < 1 << 31:
        raise NsofValueError(f"{who}: refractory_us = {refractory_us} must be in [0, 2^31)", _lib.NSOF_EINVAL)
    first_frame = _whole(who, "first_frame", first_frame)
    if first_frame < 0 or first_frame + n > 1 << 62:
        raise NsofValueError(f"{who}: first_frame = {first_frame} with {n} frames: frame indices lie in [0, 2^62]", _lib.NSOF_EINVAL)
    out = dict(refractory_us=refractory_us, seed=0, first_frame=first_frame, rate_on_q=0, rate_off_q=0, plane=None, t_ok=None)
    if noise is not None:
        if not isinstance(noise, dict) or "seed" not in noise or any(k not in NOISE_KEYS for k in noise):
            raise NsofValueError(f"{who}: noise = {noise!r}; a dict with 'seed' and rates ('rate_hz', or 'rate_on_hz' / 'rate_off_hz', or "
                                 "'rate_maps') expected", _lib.NSOF_EINVAL)
        seed = noise["seed"]
        if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 1 << 64:
            raise NsofValueError(f"{who}: noise['seed'] = {seed!r} is not a whole number in [0, 2^64)", _lib.NSOF_EINVAL)
        out["seed"] = int(seed)
        ways = [k for k in ("rate_hz", "rate_maps") if k in noise] + (["rate_on_hz / rate_off_hz"] if "rate_on_hz" in noise or
                                                                      "rate_off_hz" in noise else [])
        if len(ways) != 1:
            raise NsofValueError(f"{who}: noise gives its rates {len(ways)} ways ({', '.join(ways) or 'none'}); one of 'rate_hz', "
                                 "'rate_on_hz' / 'rate_off_hz', 'rate_maps' expected", _lib.NSOF_EINVAL)
        if "rate_maps" in noise:
            out["plane"] = _units_plane(who, _RATE, "rate_maps", noise["rate_maps"], h, w)
        elif "rate_hz" in noise:
            out["rate_on_q"] = out["rate_off_q"] = _units(who, _RATE, "rate_hz", noise["rate_hz"])
        else:
            out["rate_on_q"] = _units(who, _RATE, "rate_on_hz", noise.get("rate_on_hz", 0))
            out["rate_off_q"] = _units(who, _RATE, "rate_off_hz", noise.get("rate_off_hz", 0))
    if t_ok is not None:
        if not isinstance(t_ok, torch.Tensor) or t_ok.dtype != torch.int64 or tuple(t_ok.shape) != (h, w) or not t_ok.is_contiguous():
            raise NsofValueError(f"{who}: t_ok must be a contiguous int64 tensor [{h}][{w}] (got {getattr(t_ok, 'dtype', type(t_ok))} "
                                 f"{tuple(getattr(t_ok, 'shape', ()))})", _lib.NSOF_ESHAPE)
        out["t_ok"] = t_ok
    if refractory_us == 0 and noise is None and t_ok is None and first_frame == 0:
        return None
    return out


def events_noise_draw(seed, pixel, frame):
    """The four 32-bit words ``c0..c3`` of the noise generator for (``seed``, ``pixel`` = y * W + x, absolute ``frame``
    index), uint32 ``[4]``: Philox4x32-10 on the counter ``(pixel, frame & 0xffffffff, frame >> 32, 0x4E534546)`` under the
    key ``(seed & 0xffffffff, seed >> 32)``, computed by the library on the host (``nsof_events_noise_draw``) -- the bits
    the kernels use.  ``c0`` / ``c1`` decide whether the ON / OFF noise event of the interval before the frame exists,
    ``c2`` / ``c3`` place it in the interval."""
    for name, v, top in (("seed", seed, 1 << 64), ("pixel", pixel, 1 << 32), ("frame", frame, (1 << 62) + 1)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < top:
            raise NsofValueError(f"events_noise_draw: {name} = {v!r} is not a whole number in [0, {top})", _lib.NSOF_EINVAL)
    out = np.empty(4, np.uint32)
    _lib.load().nsof_events_noise_draw(int(seed), int(pixel), int(frame), out.ctypes.data)
    return out


def _polarity_arg(who, name, v):
    v = _whole(who, name, v)
    if not -128 <= v <= 127:
        raise NsofValueError(f"{who}: {name} = {v} does not fit an int8", _lib.NSOF_EINVAL)
    return v


def events_from_frames_dev(frames, times_us=None, *, frame_us=None, threshold=10.0, threshold_off=None, threshold_maps=None,
                           response=None, ref=None, timestamps="linear", p_on=1, p_off=-1, refractory_us=0, noise=None, t_ok=None,
                           first_frame=0, ctx=None):
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
    ``threshold_maps`` plane, is covered here: with ``threshold_maps`` the call ends in ``ctx.synchronize()``.

    The sensor model (``nsof_events_from_frames_sensor_*_dev``; all four arguments at their defaults: the plain generator
    and exactly the result above).  Every pixel also keeps ``t_ok``, the earliest time at which it may fire again.
    ``refractory_us`` (whole, [0, 2^31)): the candidates of a pixel and frame are taken in the order (t, signal before ON
    noise before OFF noise); one is emitted iff ``t >= t_ok``, and then ``t_ok = t + refractory_us``.  ``r`` moves by every
    crossing whether or not its event survives, so ``ref`` does not depend on these arguments.  ``noise``: a dict with
    ``seed`` (whole, [0, 2^64)) and the background-activity rates in Hz, given one way: ``rate_hz`` (both polarities),
    ``rate_on_hz`` / ``rate_off_hz``, or ``rate_maps`` (``[H][W][2]``, array or tensor, checked and converted on the host
    like ``threshold_maps``: hot pixels); a rate is held as ``round(rate * 2^32 / 10^6)``, which must be below 2^32.  In the
    interval before every frame but the call's first a pixel draws one Philox block (``events_noise_draw``): an ON noise
    event exists iff ``c0 < min(2^32 - 1, rate_on_q * (T[k] - T[k-1]))``, stamped ``T[k]`` (``"frame"``) or ``T[k-1] + ((c2 *
    (T[k] - T[k-1])) >> 32)`` (``"linear"``); OFF likewise with ``c1`` and ``c3``.  A rate above one event per interval
    saturates at one noise event per pixel, polarity and interval; noise does not move ``r``; a noise event comes after
    the signal events of its pixel, frame and polarity.  ``first_frame`` is the absolute index of ``frames[0]`` (the noise
    counter), ``t_ok`` the ``t_ok`` of a previous result: ``frames[0:k+1]`` with ``first_frame=f`` and then ``frames[k:n]``
    with ``first_frame=f+k`` and the first call's ``ref`` and ``t_ok`` give the one-shot stream, ``ref`` and ``t_ok`` bit for
    bit.  The result then also carries ``t_ok`` (int64 CUDA ``[H][W]``; a pixel that never fired holds the smallest int64).
    With ``"linear"`` stamps and a refractory time or a ``t_ok`` the crossings of a step are walked one by one, and a pixel
    that crosses 2^20 thresholds or more in one step is refused (``NSOF_EUNSUPPORTED``).  ``t_ok`` must stay an int64: with
    ``refractory_us > 0`` a last time above ``2^63 - 1 - refractory_us`` is refused (``NSOF_EINVAL``, before any device work);
    without a refractory time, and for the plain generator, any int64 times are taken.  With ``rate_maps`` the call ends
    in ``ctx.synchronize()``, like ``threshold_maps``."""
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
    c_on = _units(who, _THRESHOLD, "threshold", threshold)
    c_off = c_on if threshold_off is None else _units(who, _THRESHOLD, "threshold_off", threshold_off)
    plane = None if threshold_maps is None else _units_plane(who, _THRESHOLD, "threshold_maps", threshold_maps, h, w)
    if timestamps not in _TIMESTAMPS:
        raise NsofValueError(f"{who}: timestamps = {timestamps!r}; 'frame' or 'linear' expected", _lib.NSOF_EINVAL)
    p_on, p_off = _polarity_arg(who, "p_on", p_on), _polarity_arg(who, "p_off", p_off)
    sensor = _sensor_args(who, n, h, w, refractory_us, noise, t_ok, first_frame)
    if sensor is not None and sensor["refractory_us"] > 0 and int(times[-1]) > INT64_MAX - sensor["refractory_us"]:
        raise NsofValueError(f"{who}: times_us[{n - 1}] = {int(times[-1])} with refractory_us = {sensor['refractory_us']}: t_ok = t + "
                             "refractory_us would pass the int64 range", _lib.NSOF_EINVAL)
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
    if sensor is not None and sensor["t_ok"] is not None and sensor["t_ok"].device != frames.device:
        raise NsofValueError(f"{who}: t_ok must be a CUDA tensor on the frames' device", _lib.NSOF_EINVAL)

    ctx = ctx or default_context()
    dev = frames.device
    lib = ctx._lib
    d_plane = None if plane is None else torch.from_numpy(plane).to(dev)
    bounds = np.empty(n + 1, np.int64)
    p_bounds = bounds.ctypes.data_as(C.c_void_p)
    mode = _TIMESTAMPS[timestamps]
    common = (ctx.ptr, dev_ptr(frames), int(frames.stride(1)), int(frames.stride(0)), n, h, w, times.ctypes.data_as(C.c_void_p),
              lut.ctypes.data_as(C.c_void_p), c_on, c_off, dev_ptr(d_plane), dev_ptr(ref_in), ref_mode)
    # the plain or the sensor pair of entries; the sensor pair takes the stamp mode and the struct in both calls
    d_rates = st = None
    count, emit, count_extra = lib.nsof_events_from_frames_count_dev, lib.nsof_events_from_frames_emit_dev, ()
    if sensor is not None:
        if sensor["plane"] is not None:
            d_rates = torch.from_numpy(sensor["plane"].view(np.int32)).to(dev)   # the bits of the uint32 plane
        st = _lib.EventsSensor(sensor["refractory_us"], sensor["seed"], sensor["first_frame"], sensor["rate_on_q"], sensor["rate_off_q"],
                               dev_ptr(d_rates), dev_ptr(sensor["t_ok"]))
        count, emit, count_extra = (lib.nsof_events_from_frames_sensor_count_dev, lib.nsof_events_from_frames_sensor_emit_dev,
                                    (mode, C.byref(st)))
    torch.cuda.synchronize(dev)   # the frames, ref, t_ok and the planes' uploads are torch's work; the library reads them on the context's stream
    try:
        ctx.check(count(*common, *count_extra, p_bounds), who)
        total = int(bounds[n])
        ref_out = torch.empty((h, w), dtype=torch.int32, device=dev)   # fresh allocations: no pending work of torch's to wait for
        out = dict(_empty_stream(total, dev), frame_bounds=bounds, ref=ref_out)
        emit_extra = ()
        if st is not None:
            out["t_ok"] = torch.empty((h, w), dtype=torch.int64, device=dev)
            emit_extra = (C.byref(st), dev_ptr(out["t_ok"]))
        ctx.check(emit(*common, p_bounds, mode, p_on, p_off, total, *(dev_ptr(out[k]) for k, _ in _STREAM), dev_ptr(ref_out),
                       *emit_extra), who)
    finally:
        if d_plane is not None or d_rates is not None:
            # the queued kernels read the uploaded planes, and torch's allocator hands a freed block to the next allocation
            # on torch's stream at once: a plane may go only when the context's stream has drained
            ctx.synchronize()
    return out


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
