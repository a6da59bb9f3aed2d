"""Synaptic accumulator: host-side mirror of /root/reference/eventsim/event_mem_sim.py.

Same names and argument meaning as the reference (``PARAMS``, ``DT``, ``REFRACTORY_US``, ``update_state(w, V, p, dt)``,
``resistance_exp(w, p)``, ``slice_indices(t, slice_us)``, ``load_events(h5_path)``, ``simulate(...)``);
the arithmetic runs in libnsof.so on the GPU.
"""
import ctypes as C
import gzip
import json
from pathlib import Path

import numpy as np

from . import _lib
from .context import default_context, dev_ptr
from .errors import NsofValueError

# event_mem_sim.py:20-34: the defaults of every ``p`` / ``params`` / ``dt`` / ``refractory_us`` argument below (the library's
# own defaults, ``nsof_accum_default_params``, hold the same values).  won / woff are kept for the metadata file; nothing reads them.
PARAMS = dict(alphaoff=1, alphaon=1, voff=-0.2, von=0.1, koff=51.03, kon=-2.91, son=0.2, soff=0.8,
              bon=-5.12, boff=3.10, Ron=163_305, Roff=2_104_377, won=1, woff=0, wini=0.5)
DT = 5e-4
THETA_EVENTS = 1
REFRACTORY_US = 800


_PARAM_KEYS = ("alphaoff", "alphaon", "voff", "von", "koff", "kon", "son", "soff", "bon", "boff", "Ron", "Roff", "wini")


def _number(name, v):
    try:
        return float(v)
    except (TypeError, ValueError):
        raise NsofValueError(f"accumulator parameter {name} = {v!r} is not a number") from None


def accum_params(params=None, dt=None, refractory_us=None):
    """The ``nsof_accum_params`` struct of a parameter mapping (``None``: ``PARAMS``), ``dt`` (``None``: ``DT``) and
    ``refractory_us`` (``None``: ``REFRACTORY_US``).  A missing key raises ``NsofValueError`` naming it; extra keys (the
    reference's ``won`` / ``woff``) are ignored.  The value checks are the library's (``NSOF_EINVAL`` before any launch)."""
    p = PARAMS if params is None else params
    try:
        missing = [k for k in _PARAM_KEYS if k not in p]
    except TypeError:
        raise NsofValueError("params must be a mapping with the keys of nsof.PARAMS") from None
    if missing:
        raise NsofValueError(f"params lacks the key {missing[0]!r}" + (f" (and {missing[1:]})" if missing[1:] else ""))
    out = _lib.AccumParams()
    for k in _PARAM_KEYS:
        setattr(out, k, _number(k, p[k]))
    out.dt = _number("dt", DT if dt is None else dt)
    r = REFRACTORY_US if refractory_us is None else refractory_us
    if isinstance(r, float) and not r.is_integer():
        raise NsofValueError(f"refractory_us = {r!r} is not a whole number of microseconds")
    try:
        out.refractory_us = int(r)
    except (TypeError, ValueError, OverflowError):
        raise NsofValueError(f"refractory_us = {r!r} is not a whole number of microseconds") from None
    return out


def event_threshold(theta_events=None, version=1):
    """Scheme 1's event-count threshold as the library takes it: ``None`` is the module's ``THETA_EVENTS``; anything but a
    whole number >= 1 (that fits an int32), or a value other than 1 with ``version=2`` -- that scheme has no count
    threshold -- raises ``NsofValueError``."""
    th = THETA_EVENTS if theta_events is None else theta_events
    whole = isinstance(th, (int, np.integer)) and not isinstance(th, (bool, np.bool_))
    if isinstance(th, (float, np.floating)) and float(th).is_integer():
        whole, th = True, int(th)
    if not whole or not 1 <= int(th) <= 2**31 - 1:
        raise NsofValueError(f"theta_events = {theta_events!r} is not a whole number of events >= 1")
    if version == 2 and int(th) != 1:
        raise NsofValueError(f"theta_events = {theta_events!r}: scheme 2 has no event-count threshold")
    return int(th)


def _plane_maps(param_maps, shape, dtype, trial_axis):
    """``(n_trials, [(key, dtype [1 or n_trials][H][W])])`` in ``_PARAM_KEYS`` order of a ``param_maps`` mapping (``None`` or
    empty: ``(1, [])``).  A plane is ``[H][W]`` or, with ``trial_axis``, ``[T][H][W]``; ``n_trials`` is the ``T`` of the 3-D
    planes, 1 when every plane is 2-D.  Raises ``NsofValueError`` -- before any context exists or the library is called -- for
    a key that is no device parameter (``won`` / ``woff``, ``dt`` and ``refractory_us`` stay scalars), a plane of the wrong
    rank or not ``shape`` (where given; ``NSOF_ESHAPE``), 3-D planes whose trial counts differ, and a non-finite value.  The
    domain of each value (``voff < 0 < von``, ...) is the library's check."""
    layout = "[H][W] or [T][H][W]" if trial_axis else "[H][W]"
    if param_maps is None:
        return 1, []
    try:
        items = dict(param_maps.items())
    except AttributeError:
        raise NsofValueError(f"param_maps must be a mapping of parameter name -> {layout} array") from None
    unknown = [k for k in items if k not in _PARAM_KEYS]
    if unknown:
        raise NsofValueError(f"param_maps: {unknown[0]!r} is not a {'per-cell' if trial_axis else 'per-pixel'} parameter (one of {', '.join(_PARAM_KEYS)})")
    out, trials = [], None
    for k in _PARAM_KEYS:
        if k not in items:
            continue
        try:
            a = np.ascontiguousarray(items[k], dtype)
        except (TypeError, ValueError):
            raise NsofValueError(f"param_maps[{k!r}] is not an array of numbers") from None
        if a.ndim not in ((2, 3) if trial_axis else (2,)) or 0 in a.shape[:-2] or (shape is not None and a.shape[-2:] != tuple(shape)):
            raise NsofValueError(f"param_maps[{k!r}] is {a.shape}, the array is {tuple(shape) if shape is not None else '[H][W]'}"
                                 + (" (with or without a leading trial axis)" if trial_axis else ""), _lib.NSOF_ESHAPE)
        if a.ndim == 3:
            if trials is not None and a.shape[0] != trials[1]:
                raise NsofValueError(f"param_maps[{k!r}] holds {a.shape[0]} trials, param_maps[{trials[0]!r}] {trials[1]}",
                                     _lib.NSOF_ESHAPE)
            trials = trials or (k, a.shape[0])
        else:
            a = a[None]
        if not np.isfinite(a).all():
            t, r, c = (int(v) for v in np.argwhere(~np.isfinite(a))[0])
            where = f" trial {t}, row {r}, column {c}" if trial_axis else f"[{r}][{c}]"
            raise NsofValueError(f"param_maps[{k!r}]{where} = {a[t, r, c]} is not finite")
        out.append((k, a))
    return (trials[1] if trials else 1), out


def param_maps_arg(param_maps, shape=None):
    """Per-pixel parameter maps as the accumulator takes them (``nsof_accum_set_param_maps``): ``[(key, float32 [H][W])]`` in
    ``_PARAM_KEYS`` order; refusals as ``_plane_maps`` states them."""
    return [(k, a[0]) for k, a in _plane_maps(param_maps, shape, np.float32, False)[1]]


def frame_param_maps_arg(param_maps, shape=None):
    """Per-cell, per-trial parameter planes as the frame-driven entries take them (``nsof_accum_frames_f64_maps*``):
    ``(n_trials, [(key, float64 [1 or n_trials][H][W])])`` in ``_PARAM_KEYS`` order.  A plane is ``[H][W]`` (shared by the
    trials) or ``[T][H][W]`` (one per trial), float32 or float64 -- read as float64, a float32 plane widened is exact;
    refusals as ``_plane_maps`` states them."""
    return _plane_maps(param_maps, shape, np.float64, True)


def trial_param_maps_arg(param_maps, shape=None):
    """Per-pixel, per-trial parameter planes as the event-driven trial run takes them (``nsof_accum_trials_dev``):
    ``(n_trials, [(key, float32 [1 or n_trials][H][W])])`` in ``_PARAM_KEYS`` order; a plane is ``[H][W]`` (shared by the
    trials) or ``[T][H][W]``.  Refusals as ``_plane_maps`` states them, and -- so that nothing reaches the device first -- the
    domain the library checks again (``voff < 0 < von``, ``son`` / ``soff`` / ``wini`` in [0, 1], ``Ron`` / ``Roff`` positive),
    naming key, trial, row, column and value."""
    trials, maps = _plane_maps(param_maps, shape, np.float32, True)
    domain = dict(voff=(lambda a: a < 0, "must be negative (voff < 0 < von)"), von=(lambda a: a > 0, "must be positive (voff < 0 < von)"),
                  Ron=(lambda a: a > 0, "must be positive"), Roff=(lambda a: a > 0, "must be positive"))
    domain.update({k: (lambda a: (a >= 0) & (a <= 1), "lies outside [0, 1]") for k in ("son", "soff", "wini")})
    for k, a in maps:
        # (the extremes decide, without a temporary of the planes' size: every value is finite here)
        if k in domain and not (domain[k][0](a.min()) and domain[k][0](a.max())):
            t, r, c = (int(v) for v in np.argwhere(~domain[k][0](a))[0])
            raise NsofValueError(f"param_maps[{k!r}] trial {t}, row {r}, column {c} = {a[t, r, c]} {domain[k][1]}")
    return trials, maps


def _frame_maps_c(n_trials, maps):
    """The ctypes arrays (keys, planes, plane_trials) of ``frame_param_maps_arg``'s result; the planes stay referenced by
    ``maps``."""
    n = max(len(maps), 1)
    keys = (C.c_int * n)(*[_PARAM_KEYS.index(k) for k, _ in maps])
    planes = (C.c_void_p * n)(*[a.ctypes.data for _, a in maps])
    counts = (C.c_int * n)(*[a.shape[0] for _, a in maps])
    return keys, planes, counts


def variability_maps(H, W, rel_sigma, params=None, seed=0, trials=None, dtype=np.float32):  # noqa: N803
    """Device-to-device variability as parameter maps (host helper; the kernels know nothing about it): for every key of
    ``rel_sigma`` the plane ``float32(p[key] * (1 + rel_sigma[key] * N(0, 1)))`` with ``p`` = ``params`` (``None``: ``PARAMS``),
    drawn from ``np.random.default_rng(seed)`` in ``_PARAM_KEYS`` order -- the result does not depend on the mapping's order --
    and clipped into the model's domain: ``voff`` / ``von`` / ``koff`` / ``kon`` keep their sign, ``son`` / ``soff`` / ``wini``
    stay in [0, 1], ``Ron`` / ``Roff`` at least the smallest positive normal float32.
    ``trials=T``: ``[T][H][W]`` planes for Monte-Carlo trials -- the ``param_maps`` of the frame-driven path
    (``simulate_frames*``) and of the event-driven trial run (``simulate_trials*``) --, trial ``t`` exactly the planes of
    ``seed + t``.  ``dtype=np.float64`` keeps the planes unrounded (the frame-driven path reads doubles), so a spread of 0
    gives the nominal value itself; the event-driven path reads float32."""
    if trials is not None:
        if not isinstance(trials, (int, np.integer)) or isinstance(trials, (bool, np.bool_)) or trials < 1:
            raise NsofValueError(f"variability_maps: trials = {trials!r} is not a whole number >= 1")
        per = [variability_maps(H, W, rel_sigma, params, seed + t, dtype=dtype) for t in range(int(trials))]
        return {k: np.stack([m[k] for m in per]) for k in per[0]}
    if np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise NsofValueError(f"variability_maps: dtype {dtype!r} is neither float32 nor float64")
    p = PARAMS if params is None else params
    unknown = [k for k in rel_sigma if k not in _PARAM_KEYS]
    if unknown:
        raise NsofValueError(f"variability_maps: {unknown[0]!r} is not a per-pixel parameter")
    rng = np.random.default_rng(seed)
    tiny = float(np.finfo(np.float32).tiny)
    out = {}
    for k in _PARAM_KEYS:
        if k not in rel_sigma:
            continue
        nominal = _number(k, p[k])
        v = nominal * (1.0 + _number(f"rel_sigma[{k!r}]", rel_sigma[k]) * rng.standard_normal((int(H), int(W))))
        if k in ("voff", "von", "koff", "kon") and nominal != 0:
            v = np.maximum(v, tiny) if nominal > 0 else np.minimum(v, -tiny)
        elif k in ("son", "soff", "wini"):
            v = np.clip(v, 0.0, 1.0)
        elif k in ("Ron", "Roff"):
            v = np.maximum(v, tiny)
        out[k] = v.astype(dtype)
    return out


def _params_dict(ap):
    """(params dict with the reference's keys, dt, refractory_us) of an ``AccumParams`` -- what the metadata file records."""
    d = {k: getattr(ap, k) for k in _PARAM_KEYS}
    return d, ap.dt, int(ap.refractory_us)


def _torch():
    import torch
    return torch


def update_state(w, V, p=PARAMS, dt=DT, *, ctx=None):  # noqa: N803
    """``update_state(w, V, p=PARAMS, dt=DT)`` of event_mem_sim.py:40-57 for float32 arrays (numpy in -> numpy out)."""
    ap = accum_params(p, dt)
    ctx = ctx or default_context()
    w = np.ascontiguousarray(w, np.float32)
    V = np.ascontiguousarray(V, np.float32)  # noqa: N806
    if w.shape != V.shape:
        raise NsofValueError(f"w {w.shape} and V {V.shape} shapes differ", _lib.NSOF_ESHAPE)
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    dw, dv = torch.from_numpy(w).to(dev), torch.from_numpy(V).to(dev)
    out = torch.empty_like(dw)
    torch.cuda.synchronize(dev)
    ctx.check(ctx._lib.nsof_accum_update_state_p_dev(ctx.ptr, C.byref(ap), dev_ptr(dw), dev_ptr(dv), dev_ptr(out), w.size),
              "update_state")
    ctx.synchronize()
    return out.cpu().numpy()


def resistance_exp(w, p=PARAMS, *, ctx=None):
    """``resistance_exp(w, p=PARAMS)`` of event_mem_sim.py:60-63, returned as float32 (as the reference stores it, :292)."""
    ap = accum_params(p)
    ctx = ctx or default_context()
    w = np.ascontiguousarray(w, np.float32)
    torch = _torch()
    dev = torch.device("cuda", ctx.device)
    dw = torch.from_numpy(w).to(dev)
    out = torch.empty_like(dw)
    torch.cuda.synchronize(dev)
    ctx.check(ctx._lib.nsof_accum_resistance_p_dev(ctx.ptr, C.byref(ap), dev_ptr(dw), dev_ptr(out), w.size), "resistance_exp")
    ctx.synchronize()
    return out.cpu().numpy()


_EVENT_ARRAYS = (("x", "int16"), ("y", "int16"), ("p", "int8"), ("t", "int64"))   # an event stream's arrays and their dtypes


def _is_cuda(v):
    return bool(getattr(v, "is_cuda", False))


def device_events(who, x, y, p, t, ctx=None):
    """Whether the event arrays of a call are a stream in HBM.  None of them a CUDA tensor: ``None``, the host path as ever
    (arrays, lists and CPU tensors).  Otherwise all four must be CUDA tensors of dtypes int16, int16, int8, int64, 1-D,
    contiguous, of one length and on one device -- ``ctx``'s, where given -- and the number of events is returned; anything
    else that holds a CUDA tensor (a mix of host and device arrays, another dtype -- nothing is converted on the device --, a
    strided view, another device) raises ``NsofValueError`` before any device work."""
    arrs = (x, y, p, t)
    if not any(_is_cuda(v) for v in arrs):
        return None
    torch = _torch()
    for (name, dtype), v in zip(_EVENT_ARRAYS, arrs):
        if not isinstance(v, torch.Tensor) or not v.is_cuda:
            raise NsofValueError(f"{who}: {name} is no CUDA tensor while another event array is (got {type(v).__name__}"
                                 f"{' on the CPU' if isinstance(v, torch.Tensor) else ''}); a stream lies on the host or in HBM, "
                                 "all four arrays of it", _lib.NSOF_EINVAL)
    for (name, dtype), v in zip(_EVENT_ARRAYS, arrs):
        if v.dtype != getattr(torch, dtype):
            raise NsofValueError(f"{who}: {name} must be an {dtype} tensor (got {v.dtype}); a device stream is not converted",
                                 _lib.NSOF_EINVAL)
        if v.dim() != 1 or v.shape != x.shape or not v.is_contiguous():
            raise NsofValueError(f"{who}: {name} must be contiguous, one-dimensional and as long as x (got {tuple(v.shape)}, strides "
                                 f"{tuple(v.stride())}, x {tuple(x.shape)})", _lib.NSOF_ESHAPE)
        if v.device != x.device:
            raise NsofValueError(f"{who}: {name} lies on {v.device}, x on {x.device}", _lib.NSOF_EINVAL)
    if ctx is not None and x.device.index != ctx.device:
        raise NsofValueError(f"{who}: the stream lies on {x.device}, the context works on cuda:{ctx.device}", _lib.NSOF_EINVAL)
    return int(x.shape[0])


def _device_stream(who, ctx, x, y, p, t, bounds):
    """The arguments of a ``*_dev`` staging entry for a stream in HBM (``device_events``), ``None`` for a host stream:
    ``(d_x, d_y, d_p, d_t, n_events, bounds, n_slices)`` -- ``bounds`` the host int64 array as a ctypes pointer that keeps
    it alive, ``n_slices`` -1 for no bound at all -- after the one ``torch.cuda.synchronize`` that lets the library read
    torch's tensors on the context's stream.  Bounds that reach outside the stream raise ``NsofValueError``."""
    n = device_events(who, x, y, p, t, ctx)
    if n is None:
        return None
    bounds = np.ascontiguousarray(bounds, np.int64)
    if bounds.ndim != 1:
        raise NsofValueError(f"{who}: the slice bounds must be one-dimensional (got {bounds.shape})", _lib.NSOF_ESHAPE)
    if bounds.size and (bounds[-1] > n or bounds[0] < 0):
        raise NsofValueError("event arrays shorter than the slice bounds")
    _torch().cuda.synchronize(x.device)
    return dev_ptr(x), dev_ptr(y), dev_ptr(p), dev_ptr(t), n, bounds.ctypes.data_as(C.c_void_p), bounds.size - 1


def _device_bounds(ctx, lib_fn, d_t, slice_us, idx, cap):
    n = int(lib_fn(ctx.ptr, dev_ptr(d_t), int(d_t.shape[0]), int(slice_us), idx, cap))
    if n < 0:
        ctx.check(n, "slice_index_array")
    return n


def slice_index_array(t, slice_us, ctx=None):
    """searchsorted(t, arange(t[0], t[-1]+slice_us, slice_us)) of event_mem_sim.py:78-83 as one int64 array (host).
    ``t``: anything array-like on the host or, for a stream in HBM, a contiguous 1-D int64 CUDA tensor on the device of
    ``ctx`` (``None``: the default context; host arrays need none) -- the bounds are then found on the device
    (``nsof_accum_slice_bounds_dev``: two calls, each waits for the context's stream once, after one
    ``torch.cuda.synchronize``) and only they come back; a ``t`` that decreases raises ``NsofValueError`` (``NSOF_EINVAL``)
    naming the first such event.  ``t`` may be freed when the call returns."""
    if _is_cuda(t):
        torch = _torch()
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or t.dim() != 1 or not t.is_contiguous():
            raise NsofValueError(f"slice_index_array: a device t must be a contiguous one-dimensional int64 tensor (got "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))})", _lib.NSOF_EINVAL)
        ctx = ctx or default_context()
        if t.device.index != ctx.device:
            raise NsofValueError(f"slice_index_array: t lies on {t.device}, the context works on cuda:{ctx.device}", _lib.NSOF_EINVAL)
        fn = ctx._lib.nsof_accum_slice_bounds_dev
        torch.cuda.synchronize(t.device)   # t is torch's work; the library reads it on the context's stream
        n = _device_bounds(ctx, fn, t, slice_us, None, 0)
        idx = np.empty(n, np.int64)
        if n:
            _device_bounds(ctx, fn, t, slice_us, idx.ctypes.data, n)
        return idx
    t = np.ascontiguousarray(t, np.int64)
    lib = _lib.load()
    n = lib.nsof_accum_slice_bounds(t.ctypes.data, t.size, int(slice_us), None, 0)
    idx = np.empty(n, np.int64)
    lib.nsof_accum_slice_bounds(t.ctypes.data, t.size, int(slice_us), idx.ctypes.data, n)
    return idx


def slice_indices(t, slice_us):
    """Generator of ``slice(start, stop)`` objects, as the reference's ``slice_indices``."""
    idx = slice_index_array(t, slice_us)
    for i in range(len(idx) - 1):
        yield slice(int(idx[i]), int(idx[i + 1]))


def bincount_2d(x, y, H, W, *, ctx=None):  # noqa: N803
    """``bincount_2d`` of event_mem_sim.py:100-104: events per pixel, int32 [H][W] (atomic adds on the GPU)."""
    ctx = ctx or default_context()
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape or x.ndim != 1:
        raise NsofValueError("bincount_2d: x and y must be 1-D arrays of one length")
    if x.size and (x.min() < -32768 or x.max() > 32767 or y.min() < -32768 or y.max() > 32767):
        raise NsofValueError("bincount_2d: coordinates outside the int16 range of /CD/events")
    x16, y16 = np.ascontiguousarray(x, np.int16), np.ascontiguousarray(y, np.int16)
    out = np.empty((int(H), int(W)), np.int32)
    ctx.check(ctx._lib.nsof_accum_bincount_2d(ctx.ptr, x16.ctypes.data, y16.ctypes.data, x16.size, int(H), int(W),
                                              out.ctypes.data), "bincount_2d")
    return out


def generate_synthetic_events(H=240, W=320, box_h=50, box_w=50, speed_pps=300, duration_s=1.5):  # noqa: N803
    """``generate_synthetic_events`` of event_mem_sim.py:109-158: a white box moving left to right; ON (+1) events
    on the pixels it newly covers, OFF (-1) on the ones it leaves, one frame every ``DT`` seconds.  Same event order
    as the reference (per step: ON pixels in row-major order, then OFF pixels).  Host generator (test input)."""
    t_step_us = int(DT * 1_000_000)
    duration_us = int(duration_s * 1_000_000)
    y0 = (H - box_h) // 2
    rows = np.arange(y0, min(y0 + box_h, H))
    rows = rows[rows >= 0]
    xs, ys, ps, ts = [], [], [], []
    prev = (0, 0)                                   # covered column range [a, b) of the previous frame
    for t_us in range(0, duration_us, t_step_us):
        start = int((t_us / 1_000_000) * speed_pps)
        end = start + box_w
        cur = (max(0, start), min(W, end)) if (start < W and end > 0) else (0, 0)
        cols_cur = np.arange(cur[0], cur[1])
        cols_prev = np.arange(prev[0], prev[1])
        for cols, pol in ((np.setdiff1d(cols_cur, cols_prev), 1), (np.setdiff1d(cols_prev, cols_cur), -1)):
            if cols.size and rows.size:
                yy, xx = np.meshgrid(rows, cols, indexing="ij")   # row-major, like np.where
                xs.append(xx.ravel()); ys.append(yy.ravel())
                ps.append(np.full(xx.size, pol)); ts.append(np.full(xx.size, t_us))
        prev = cur
    if not xs:
        e = np.array([], dtype=int)
        return e, e.copy(), e.copy(), e.copy()
    return (np.concatenate(xs).astype(int), np.concatenate(ys).astype(int), np.concatenate(ps).astype(int),
            np.concatenate(ts).astype(int))


def load_events(h5_path):
    """``load_events`` of event_mem_sim.py:69-75 (needs h5py; sensor size inferred from the data)."""
    import h5py
    with h5py.File(h5_path, "r") as f:
        evs = f["/CD/events"]
        x, y, p, t = evs["x"][:], evs["y"][:], evs["p"][:].astype(int), evs["t"][:]
    H, W = int(y.max()) + 1, int(x.max()) + 1  # noqa: N806
    return x, y, p, t, H, W


class Accumulator:
    """Device-resident array state (w, refractory maps) that can be advanced chunk by chunk.

    ``params`` (a mapping with the keys of ``PARAMS``), ``dt`` and ``refractory_us`` give the device the array is made of
    (``None``: the module's ``PARAMS`` / ``DT`` / ``REFRACTORY_US``); they are fixed for the accumulator's life and read
    back as ``self.params`` / ``self.dt`` / ``self.refractory_us``.  ``theta_events`` (``None``: ``THETA_EVENTS``) is scheme
    1's event-count threshold: a pixel pulses in a slice that holds at least that many of its events (read back as
    ``self.theta_events``).  ``param_maps`` (a mapping key of ``PARAMS`` -> array-like [H][W], read as float32) makes those
    parameters per pixel -- an array of devices that differ (``variability_maps``); the other keys keep their scalar, and
    ``self.param_maps`` reads the planes back."""

    def __init__(self, height, width, version=1, polarity="split", active_v=-8.0, silent_v=0.0, *, ctx=None,
                 dense=None, frames_path=None, params=None, dt=None, refractory_us=None, theta_events=None, param_maps=None):
        ap = accum_params(params, dt, refractory_us)
        theta = event_threshold(theta_events, version)
        maps = param_maps_arg(param_maps, (int(height), int(width)))
        if version not in (1, 2):
            raise NsofValueError("version must be 1 or 2")
        if polarity not in ("split", "magnitude"):
            raise NsofValueError("polarity must be 'split' or 'magnitude'")
        self.ctx = ctx or default_context()
        self.H, self.W, self.version = int(height), int(width), version
        self.split = version == 2 and polarity == "split"
        p = C.c_void_p()
        self.ctx.check(self.ctx._lib.nsof_accum_create_p(self.ctx.ptr, self.H, self.W, version, int(self.split),
                                                         float(active_v), float(silent_v), C.byref(ap), C.byref(p)),
                       "accum_create")
        self._p = p
        used = _lib.AccumParams()
        self.ctx.check(self.ctx._lib.nsof_accum_get_params(self._p, C.byref(used)), "accum_get_params")
        self.params, self.dt, self.refractory_us = _params_dict(used)
        if theta != 1:
            self.ctx.check(self.ctx._lib.nsof_accum_set_event_threshold(self._p, theta), "accum_set_event_threshold")
        if dense is not None:   # None: automatic; True: the every-pixel pass; False: the event-pixel update where it is exact
            self.ctx.check(self.ctx._lib.nsof_accum_set_dense(self._p, 1 if dense else -1), "accum_set_dense")
        if frames_path is not None:   # run_frames: "tiles" (default where it applies) or "copy_patch"
            self.ctx.check(self.ctx._lib.nsof_accum_set_frames_path(self._p, {"tiles": 0, "copy_patch": 1}[frames_path]),
                           "accum_set_frames_path")
        if maps:
            try:
                self._set_maps(maps)
            except Exception:
                self.close()
                raise

    def _set_maps(self, maps):
        keys = (C.c_int * len(maps))(*[_PARAM_KEYS.index(k) for k, _ in maps])
        planes = (C.c_void_p * len(maps))(*[a.ctypes.data for _, a in maps])
        self.ctx.check(self.ctx._lib.nsof_accum_set_param_maps(self._p, len(maps), keys, planes), "accum_set_param_maps")

    def set_param_maps(self, param_maps):
        """Replace the per-pixel parameter maps (``None`` or empty: back to the uniform device) and reset the array
        (``nsof_accum_set_param_maps``); accepted only before the first slice or right after ``reset()``."""
        self._set_maps(param_maps_arg(param_maps, (self.H, self.W)))

    @property
    def param_maps(self):
        """The per-pixel parameter maps in use, ``{key: float32 [H][W]}`` (empty for a uniform device)."""
        mask = C.c_uint()
        self.ctx.check(self.ctx._lib.nsof_accum_param_map_mask(self._p, C.byref(mask)), "accum_param_map_mask")
        out = {}
        for i, k in enumerate(_PARAM_KEYS):
            if mask.value >> i & 1:
                out[k] = np.empty((self.H, self.W), np.float32)
                self.ctx.check(self.ctx._lib.nsof_accum_read_param_map(self._p, i, out[k].ctypes.data), "accum_read_param_map")
        return out

    @property
    def theta_events(self):
        """Scheme 1's event-count threshold this accumulator runs with (``nsof_accum_get_event_threshold``)."""
        th = C.c_int()
        self.ctx.check(self.ctx._lib.nsof_accum_get_event_threshold(self._p, C.byref(th)), "accum_get_event_threshold")
        return th.value

    def reset(self):
        self.ctx.check(self.ctx._lib.nsof_accum_reset(self._p), "accum_reset")

    def step(self, x, y, p, t, bounds, snap_every=0):
        """Advance over slices ``[bounds[i], bounds[i+1])`` of the event arrays: host arrays, or -- a stream in HBM -- four
        CUDA tensors as ``device_events`` takes them (``nsof_accum_step_events_dev``: checked on the device, copied device
        to device, the same state and snapshots bit for bit; ``bounds`` stays a host array).  The device form waits for the
        device once before the library reads the tensors and returns when they have been copied: the caller may free or
        overwrite them then."""
        dev = _device_stream("Accumulator.step", self.ctx, x, y, p, t, bounds)
        if dev is not None:
            if dev[-1] >= 1:
                self.ctx.check(self.ctx._lib.nsof_accum_step_events_dev(self._p, *dev, int(snap_every)), "accum_step_events")
            return
        x = np.ascontiguousarray(x, np.int16)
        y = np.ascontiguousarray(y, np.int16)
        p = np.ascontiguousarray(p, np.int8)
        t = np.ascontiguousarray(t, np.int64)
        bounds = np.ascontiguousarray(bounds, np.int64)
        if bounds.size < 2:
            return
        if bounds[-1] > x.size or not (x.size == y.size == p.size == t.size):
            raise NsofValueError("event arrays shorter than the slice bounds")
        self.ctx.check(self.ctx._lib.nsof_accum_step_events(self._p, x.ctypes.data, y.ctypes.data, p.ctypes.data,
                                                            t.ctypes.data, bounds.ctypes.data, bounds.size - 1,
                                                            int(snap_every)), "accum_step_events")

    def set_events(self, x, y, p, t, bounds):
        """Upload the events of all slices once (``nsof_accum_set_events``); ``run`` then advances over sub-ranges.  Four CUDA
        tensors (``device_events``) are staged where they lie (``nsof_accum_set_events_dev``), as ``step`` takes them: the
        accumulator keeps its own copy, so the tensors may be freed when the call returns."""
        dev = _device_stream("Accumulator.set_events", self.ctx, x, y, p, t, bounds)
        if dev is not None:
            if dev[-1] < 0:
                raise NsofValueError("event arrays shorter than the slice bounds")
            self.n_staged = dev[-1]
            self.ctx.check(self.ctx._lib.nsof_accum_set_events_dev(self._p, *dev), "accum_set_events")
            return
        x = np.ascontiguousarray(x, np.int16)
        y = np.ascontiguousarray(y, np.int16)
        p = np.ascontiguousarray(p, np.int8)
        t = np.ascontiguousarray(t, np.int64)
        bounds = np.ascontiguousarray(bounds, np.int64)
        if bounds.size < 1 or bounds[-1] > x.size or not (x.size == y.size == p.size == t.size):
            raise NsofValueError("event arrays shorter than the slice bounds")
        self.n_staged = bounds.size - 1
        self.ctx.check(self.ctx._lib.nsof_accum_set_events(self._p, x.ctypes.data, y.ctypes.data, p.ctypes.data,
                                                           t.ctypes.data, bounds.ctypes.data, bounds.size - 1),
                       "accum_set_events")

    def set_slice_times(self, t_first, t_last):
        """Scheme 2 on a row band: the first / last event time of every slice of the WHOLE stream
        (``nsof_accum_set_slice_times``; ``nsof.dist.global_slice_times``) in place of those of the staged band events."""
        t_first = np.ascontiguousarray(t_first, np.int64)
        t_last = np.ascontiguousarray(t_last, np.int64)
        if t_first.shape != t_last.shape or t_first.ndim != 1:
            raise NsofValueError("t_first / t_last: one entry per staged slice")
        self.ctx.check(self.ctx._lib.nsof_accum_set_slice_times(self._p, t_first.ctypes.data, t_last.ctypes.data, t_first.size),
                       "accum_set_slice_times")

    def run(self, first_slice, n_slices, snap_every=0):
        self.ctx.check(self.ctx._lib.nsof_accum_run(self._p, int(first_slice), int(n_slices), int(snap_every)),
                       "accum_run")

    def run_surface(self, first_slice, n_slices, d_out, which=0, row_stride=None, mode="state"):
        """``run`` + ``surface_u8`` of the state after the last slice as one call (``nsof_accum_run_surface``): the dense
        scheme-1 update's last pass writes the frame itself -- same bytes as the two calls, one pass over the array less."""
        self.ctx.check(self.ctx._lib.nsof_accum_run_surface(self._p, int(first_slice), int(n_slices), which,
                                                            {"current": 0, "state": 1}[mode], dev_ptr(d_out),
                                                            self.W if row_stride is None else int(row_stride)),
                       "accum_run_surface")

    def run_frames(self, first_slice, n_frames, every, frames, which=0, mode="state"):
        """``n_frames`` intervals of ``every`` slices, the surface after each into ``frames[k]`` (uint8 CUDA tensor [n][H][W]):
        one call (``nsof_accum_run_frames``).  Scheme 1 with ``silent_v`` in the dead zone (and ``dense`` not forced): frame
        k is frame k-1 copied and patched at the event pixels -- byte-identical to ``run_surface`` per interval."""
        if int(frames.stride(2)) != 1:
            raise NsofValueError("frames: pixel stride must be 1")
        self.ctx.check(self.ctx._lib.nsof_accum_run_frames(self._p, int(first_slice), int(n_frames), int(every), which,
                                                           {"current": 0, "state": 1}[mode], dev_ptr(frames),
                                                           int(frames.stride(1)), int(frames.stride(0)) if n_frames > 1 else 0),
                       "accum_run_frames")

    def surface_u8(self, d_out, which=0, row_stride=None, mode="state"):
        """The current surface as an 8-bit frame written to DEVICE memory (torch uint8 tensor / address).
        ``mode``: "current" = the reference's current -> gray map (optical_flow_seg.py:426-431; saturates at 255 for
        w >= 0.42), "state" = uint8(255 * w)."""
        self.ctx.check(self.ctx._lib.nsof_accum_surface_u8_dev(self._p, which, {"current": 0, "state": 1}[mode],
                                                               dev_ptr(d_out),
                                                               self.W if row_stride is None else int(row_stride)),
                       "accum_surface_u8")

    def surface_f32(self, d_out, which=0, row_stride=None, mode="state"):
        """The same surface as a float32 frame in DEVICE memory (torch float32 tensor / address; ``row_stride`` in BYTES,
        default 4 * W): the value ``surface_u8`` truncates to 8 bits, clipped to [0, 255] and rounded to float instead
        (``nsof_accum_surface_f32_dev``).  Always finite: the unquantised input of ``farneback_sequence``."""
        if d_out is not None and getattr(d_out, "dtype", None) is not None and str(d_out.dtype) != "torch.float32":
            raise NsofValueError(f"surface_f32 writes float32 (got {d_out.dtype})")
        self.ctx.check(self.ctx._lib.nsof_accum_surface_f32_dev(self._p, which, {"current": 0, "state": 1}[mode],
                                                                dev_ptr(d_out),
                                                                4 * self.W if row_stride is None else int(row_stride)),
                       "accum_surface_f32")

    def block_current(self, memsize, which=0, snapshot=-1, v_ds=1.0):
        """Block maximum of the device current ``v_ds / R`` over ``memsize x memsize`` pixel blocks, float64
        [H // memsize][W // memsize], reduced on the GPU (``nsof_accum_block_current``): the input of the gating image
        (``current_to_gray``) without downloading the surface.  ``snapshot`` >= 0 takes a stored snapshot (not
        consumed), -1 the current state."""
        out = np.empty((self.H // int(memsize), self.W // int(memsize)), np.float64)
        self.ctx.check(self.ctx._lib.nsof_accum_block_current(self._p, int(which), int(snapshot), int(memsize),
                                                              float(v_ds), out.ctypes.data), "accum_block_current")
        return out

    def block_current_dev(self, memsize, d_out, which=0, snapshot=-1, v_ds=1.0):
        """``block_current`` written to DEVICE memory (``d_out``: torch float64 tensor / address of
        (H // memsize) * (W // memsize) doubles), asynchronous: the input of ``gating.roi_from_surface_dev``."""
        self.ctx.check(self.ctx._lib.nsof_accum_block_current_dev(self._p, int(which), int(snapshot), int(memsize),
                                                                  float(v_ds), dev_ptr(d_out)), "accum_block_current_dev")

    def state(self, which=0):
        """-> dict(w float32 [H][W], next_ok int64 [H][W], slice_counter) -- everything a resume needs."""
        w = np.empty((self.H, self.W), np.float32)
        nok = np.empty((self.H, self.W), np.int64)
        cnt = C.c_int64()
        self.ctx.check(self.ctx._lib.nsof_accum_read_state(self._p, which, w.ctypes.data, nok.ctypes.data,
                                                           C.byref(cnt)), "accum_read_state")
        return dict(w=w, next_ok=nok, slice_counter=cnt.value)

    def load_state(self, state, which=0):
        """Inverse of ``state()`` (e.g. ``w_final`` of a stored run: ``load_state(dict(w=w_final, slice_counter=n))``)."""
        w = np.ascontiguousarray(state["w"], np.float32)
        if w.shape != (self.H, self.W):
            raise NsofValueError(f"state is {w.shape}, the array is {(self.H, self.W)}")
        nok = state.get("next_ok")
        nok = None if nok is None else np.ascontiguousarray(nok, np.int64)
        self.ctx.check(self.ctx._lib.nsof_accum_write_state(self._p, which, w.ctypes.data,
                                                            None if nok is None else nok.ctypes.data,
                                                            int(state.get("slice_counter", 0))), "accum_write_state")

    def w(self, which=0):
        out = np.empty((self.H, self.W), np.float32)
        self.ctx.check(self.ctx._lib.nsof_accum_read_w(self._p, which, out.ctypes.data), "accum_read_w")
        return out

    def resistance(self, which=0):
        out = np.empty((self.H, self.W), np.float32)
        self.ctx.check(self.ctx._lib.nsof_accum_read_resistance(self._p, which, out.ctypes.data), "accum_read_R")
        return out

    def snapshot_count(self):
        return int(self.ctx._lib.nsof_accum_snapshot_count(self._p))

    def snapshots(self):
        """-> list (one per array) of float32 [count][H][W]; clears the device ring."""
        n = self.ctx._lib.nsof_accum_snapshot_count(self._p)
        outs = []
        for which in range(2 if self.split else 1):
            out = np.empty((n, self.H, self.W), np.float32)
            self.ctx.check(self.ctx._lib.nsof_accum_read_snapshots(self._p, which, out.ctypes.data, n),
                           "accum_read_snapshots")
            outs.append(out)
        return outs

    def close(self):
        if getattr(self, "_p", None) is not None:
            self.ctx._lib.nsof_accum_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def simulate(events, version=1, slice_us=1_000, active_v=-8.0, silent_v=0.0, save_video=False, polarity="split",
             *, sensor_size=None, out_prefix=None, ctx=None, dense=None, params=None, dt=None, refractory_us=None,
             theta_events=None, param_maps=None):
    """``simulate`` of event_mem_sim.py:164-286.

    ``events``: an HDF5 path with a ``/CD/events`` group (as the reference) or a tuple ``(x, y, p, t)`` of arrays.
    Returns ``dict(w_final, resistances[, w_final_b, resistances_b])`` with the reference's snapshot cadence
    (every ``max(1, nslices // 100)`` slices).  With ``out_prefix`` (or an HDF5 path) the same
    ``.V{version}.npz`` / ``.V2_b.npz`` / ``.json.gz`` files as the reference (:289-322) are written.
    ``save_video`` is accepted for signature compatibility; MP4 previews are not produced.
    ``params`` / ``dt`` / ``refractory_us``: the device model, as for ``Accumulator`` (the reference reads its module
    globals ``PARAMS`` / ``REFRACTORY_US`` and ``update_state``'s default ``dt``).  ``theta_events``: scheme 1's event-count
    threshold (the reference's module global ``THETA_EVENTS``; ``None`` = this module's).  The metadata file records the
    values that were used.  ``param_maps``: per-pixel parameters, as for ``Accumulator``; the ``.npz`` then also holds the planes
    as ``map_<key>`` and the metadata lists their keys as ``param_maps``.
    """
    if version not in (1, 2):
        raise NsofValueError("version must be 1 or 2")
    if polarity not in ("split", "magnitude"):
        raise NsofValueError("polarity must be 'split' or 'magnitude'")
    accum_params(params, dt, refractory_us)   # a missing key is reported before the events are read
    theta = event_threshold(theta_events, version)
    maps = param_maps_arg(param_maps)   # ... and so are a wrong key or a non-finite value (the shape: once the sensor is known)
    h5_path = None
    if isinstance(events, (str, Path)):
        h5_path = Path(events)
        x, y, p, t, H, W = load_events(h5_path)  # noqa: N806
    else:
        x, y, p, t = events
        x, y, t = np.asarray(x), np.asarray(y), np.asarray(t)
        if x.size == 0:
            raise NsofValueError("empty event stream")
        if sensor_size is None:
            H, W = int(y.max()) + 1, int(x.max()) + 1  # noqa: N806  (event_mem_sim.py:74)
        else:
            H, W = sensor_size  # noqa: N806
    maps = param_maps_arg(dict(maps), (int(H), int(W)))
    idx = slice_index_array(t, slice_us)
    nslices = max(len(idx) - 1, 0)
    every = max(1, nslices // 100)
    acc = Accumulator(H, W, version, polarity, active_v, silent_v, ctx=ctx, dense=dense, params=params, dt=dt,
                      refractory_us=refractory_us, **({} if theta_events is None else dict(theta_events=theta)),
                      **(dict(param_maps=dict(maps)) if maps else {}))
    # what the metadata file records: the model this run uses, written with the caller's own numbers (the accumulator holds
    # the same values as doubles; the defaults stay the integers the reference writes), plus won / woff, which nothing reads
    src = PARAMS if params is None else params
    used = ({k: src.get(k, PARAMS[k]) for k in PARAMS}, DT if dt is None else dt,
            REFRACTORY_US if refractory_us is None else int(refractory_us))
    try:
        acc.step(x, y, p, t, idx, snap_every=every)
        snaps = acc.snapshots()
        out = dict(w_final=acc.w(0), resistances=snaps[0])
        if acc.split:
            out.update(w_final_b=acc.w(1), resistances_b=snaps[1])
    finally:
        acc.close()
    prefix = Path(out_prefix) if out_prefix is not None else h5_path
    if prefix is not None:
        _save_outputs(prefix, out, version, slice_us, polarity, h5_path, *used, theta_events=theta, param_maps=maps)
    return out


def c2c_arg(c2c):
    """Cycle-to-cycle write noise as the trial run takes it: ``None`` stays ``None``; a mapping with ``sigma`` (both
    directions) or ``sigma_on`` / ``sigma_off`` (a missing one is 0) and ``seed`` (default 0) becomes ``(seed, sigma_on,
    sigma_off)``.  Raises ``NsofValueError`` -- nothing else is touched -- for anything but a mapping, an unknown key, ``sigma``
    together with a directional key, a spread that is no number, negative or not finite, and a seed that is no whole
    number in ``[0, 2**64)``."""
    if c2c is None:
        return None
    try:
        items = dict(c2c.items())
    except AttributeError:
        raise NsofValueError("c2c must be a mapping with the keys sigma or sigma_on / sigma_off, and seed") from None
    unknown = [k for k in items if k not in ("sigma", "sigma_on", "sigma_off", "seed")]
    if unknown:
        raise NsofValueError(f"c2c: {unknown[0]!r} is not one of sigma, sigma_on, sigma_off, seed")
    if "sigma" in items and ("sigma_on" in items or "sigma_off" in items):
        raise NsofValueError("c2c: sigma sets both directions; give it, or sigma_on / sigma_off, not both")

    def spread(name):
        v = items.get("sigma", 0.0) if "sigma" in items else items.get(name, 0.0)
        name = "sigma" if "sigma" in items else name
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise NsofValueError(f"c2c[{name!r}] = {v!r} is not a number")
        if not np.isfinite(v) or v < 0:
            raise NsofValueError(f"c2c[{name!r}] = {v!r} is not a finite number >= 0")
        return float(v)
    sigma_on, sigma_off = spread("sigma_on"), spread("sigma_off")
    seed = items.get("seed", 0)
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2**64:
        raise NsofValueError(f"c2c['seed'] = {seed!r} is not a whole number in [0, 2**64)")
    return int(seed), sigma_on, sigma_off


def c2c_noise(seed, array, trial, pixel, first_slice, n):
    """The standard variates of the trial run's cycle-to-cycle noise, float32 ``[n]``: xi of (``seed``, ``array`` 0 / 1,
    ``trial``, ``pixel`` = y * W + x, slice ``first_slice + i``) -- Philox4x32-10 and a 16-byte Irwin-Hall sum, computed by the
    library on the host (``nsof_accum_c2c_noise``): the bits the kernels use.  For the frame-driven run
    (``simulate_frames*(c2c=)``): ``array`` = 0, ``pixel`` is the cell ``r * W + c`` of the compressed grid and ``first_slice``
    the pair index (``first_pair + f``)."""
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2**64:
        raise NsofValueError(f"seed = {seed!r} is not a whole number in [0, 2**64)")
    if array not in (0, 1) or not 0 <= int(trial) < 65535 or not 0 <= int(pixel) < 2**32 or not 0 <= int(first_slice) < 2**63 or int(n) < 0:
        raise NsofValueError(f"c2c_noise: array {array!r} (0 or 1), trial {trial!r} (0..65534), pixel {pixel!r} (< 2**32), first_slice "
                             f"{first_slice!r} or n {n!r} out of range")
    out = np.empty(int(n), np.float32)
    _lib.load().nsof_accum_c2c_noise(int(seed), int(array), int(trial), int(pixel), int(first_slice), int(n), out.ctypes.data)
    return out


def trial_voltage_arg(name, v, trials):
    """A drive voltage of the trial run as the library takes it: a number -> float32 ``[1]`` (all trials), a sequence of
    ``trials`` numbers -> float32 ``[trials]`` (one per trial).  Raises ``NsofValueError`` for a sequence of another length,
    a value that is no number, and one that is not a finite float32."""
    def num(u, where):
        if isinstance(u, (bool, np.bool_)) or not isinstance(u, (int, float, np.integer, np.floating)):
            raise NsofValueError(f"{name}{where} = {u!r} is not a number")
        with np.errstate(over="ignore"):
            f = np.float32(u)
        if not np.isfinite(u) or not np.isfinite(f):
            raise NsofValueError(f"{name}{where} = {u!r} is not a finite float32")
        return f
    if isinstance(v, np.ndarray) and v.ndim == 0:
        v = v.item()
    if isinstance(v, (str, bytes)) or np.ndim(v) == 0:
        return np.array([num(v, "")], np.float32)
    if np.ndim(v) != 1:
        raise NsofValueError(f"{name} is neither a number nor a sequence of {trials} numbers (one per trial)")
    seq = list(v)
    if len(seq) != trials:
        raise NsofValueError(f"{name} holds {len(seq)} voltages, the run has {trials} trials", _lib.NSOF_ESHAPE)
    return np.array([num(u, f"[{i}]") for i, u in enumerate(seq)], np.float32)


def _trial_scalars(version, polarity, params, dt, refractory_us, theta_events, c2c, trials):
    """What the trial run checks before it looks at the sensor or the events -> dict(version, split, ap, theta, noise)."""
    if version not in (1, 2):
        raise NsofValueError("version must be 1 or 2")
    if polarity not in ("split", "magnitude"):
        raise NsofValueError("polarity must be 'split' or 'magnitude'")
    ap = accum_params(params, dt, refractory_us)
    theta = event_threshold(theta_events, version)
    noise = c2c_arg(c2c)
    if trials is not None and (not isinstance(trials, (int, np.integer)) or isinstance(trials, (bool, np.bool_)) or trials < 1):
        raise NsofValueError(f"trials = {trials!r} is not a whole number >= 1")
    return dict(version=version, split=version == 2 and polarity == "split", ap=ap, theta=theta, noise=noise)


def _trial_config(early, H, W, param_maps, active_v, silent_v, trials, snapshot_every, memsize, v_ds):  # noqa: N803
    """... and what it checks once the sensor is known: the planes, the trial count, the voltages, the block currents.
    Everything ``TrialAccumulator`` hands to ``nsof_accum_trials_create``; no context is touched."""
    n_trials, maps = trial_param_maps_arg(param_maps, (H, W))
    if trials is not None:
        for k, a in maps:   # (a 2-D plane arrives here as [1][H][W]: shared by the trials)
            if np.ndim(param_maps[k]) == 3 and a.shape[0] != trials:
                raise NsofValueError(f"param_maps[{k!r}] holds {a.shape[0]} trials, trials = {trials}", _lib.NSOF_ESHAPE)
        n_trials = int(trials)
    v_act, v_sil = trial_voltage_arg("active_v", active_v, n_trials), trial_voltage_arg("silent_v", silent_v, n_trials)
    for name, v in (("snapshot_every", snapshot_every), ("memsize", memsize)):
        if v is not None and (not isinstance(v, (int, np.integer)) or isinstance(v, (bool, np.bool_)) or v < 1):
            raise NsofValueError(f"{name} = {v!r} is not a whole number >= 1")
    if memsize is not None and memsize > min(H, W):
        raise NsofValueError(f"memsize = {memsize} is larger than the {H}x{W} sensor")
    if memsize is not None and snapshot_every is None:
        raise NsofValueError("memsize needs snapshot_every: the cadence of the block currents is fixed for the object's life")
    if not v_ds > 0:
        raise NsofValueError(f"v_ds = {v_ds!r} must be positive")
    return dict(early, H=int(H), W=int(W), n_trials=n_trials, maps=maps, v_act=v_act, v_sil=v_sil,
                every=1 if snapshot_every is None else int(snapshot_every), memsize=None if memsize is None else int(memsize),
                v_ds=float(v_ds))


class TrialAccumulator:
    """The Monte-Carlo trial run as a device-resident object (``nsof_accum_trials``): the ``T`` states, the refractory maps
    and the slice counter stay in HBM and the stream is handed over chunk by chunk, so a recording of any length runs, the
    state can be read out between chunks, and each trial may have its own drive voltages.

    ``param_maps`` / ``trials`` / ``c2c`` and the device arguments as for ``simulate_trials_dev``.  ``active_v`` / ``silent_v``: a
    number, or a sequence of ``T`` numbers -- trial ``t`` writes with ``active_v[t]`` and leaks with ``silent_v[t]``
    (``version=2`` drives with the float32 sum of the two).  ``memsize`` (with ``snapshot_every`` and ``v_ds``, all fixed for
    the object's life) makes ``step`` return block currents.  A run cut into chunks at any slices equals the run in one
    chunk bit for bit, noise included: groups and snapshots follow the absolute slice counter, and a noise variate is a
    function of the absolute slice index.  Trial ``t`` equals ``Accumulator(param_maps=planes[t], active_v=active_v[t], ...)``
    stepped over the same slices bit for bit.  Every refusal of the arguments comes before a context exists."""

    def __init__(self, height, width, param_maps, version=1, polarity="split", active_v=-8.0, silent_v=0.0, *, trials=None,
                 c2c=None, params=None, dt=None, refractory_us=None, theta_events=None, snapshot_every=None, memsize=None, v_ds=1.0,
                 ctx=None, _config=None):
        self._p = None
        cfg = _config or _trial_config(_trial_scalars(version, polarity, params, dt, refractory_us, theta_events, c2c, trials),
                                       int(height), int(width), param_maps, active_v, silent_v, trials, snapshot_every, memsize, v_ds)
        self.H, self.W, self.version, self.split = cfg["H"], cfg["W"], cfg["version"], cfg["split"]
        self.trials, self.arrays, self.memsize, self.snapshot_every = cfg["n_trials"], 2 if cfg["split"] else 1, cfg["memsize"], cfg["every"]
        self.ctx = ctx or default_context()
        maps, noise = cfg["maps"], cfg["noise"]
        p = C.c_void_p()
        self.ctx.check(self.ctx._lib.nsof_accum_trials_create(
            self.ctx.ptr, self.H, self.W, self.version, int(self.split), C.byref(cfg["ap"]), cfg["theta"], self.trials, len(maps),
            *_frame_maps_c(self.trials, maps), None if noise is None else C.byref(_lib.AccumC2c(*noise)), cfg["v_act"].ctypes.data,
            cfg["v_act"].size, cfg["v_sil"].ctypes.data, cfg["v_sil"].size, self.snapshot_every, self.memsize or 0, cfg["v_ds"],
            C.byref(p)), "accum_trials_create")
        self._p = p

    @property
    def _h(self):
        if self._p is None:
            raise NsofValueError("the trial accumulator is closed")
        return self._p

    def _empty(self, shape, dtype):
        torch = _torch()
        dev = torch.device("cuda", self.ctx.device)
        out = torch.empty(shape, dtype=dtype, device=dev)
        torch.cuda.synchronize(dev)   # the library writes on the context's stream
        return out

    @property
    def slice_counter(self):
        """The slices run since creation, ``reset()`` or the loaded state's own count."""
        cnt = C.c_int64()
        self.ctx.check(self.ctx._lib.nsof_accum_trials_read_state(self._h, None, None, C.byref(cnt)), "accum_trials_read_state")
        return cnt.value

    def step(self, x, y, p, t, bounds):
        """Advance over slices ``[bounds[i], bounds[i+1])`` of the event arrays (synchronous).  With ``memsize``: returns
        the float64 CUDA tensor ``[A][T][S][H // memsize][W // memsize]`` of the block currents after the ``S`` snapshot slices
        -- absolute indices 0, ``snapshot_every``, ... -- inside this chunk (the chunks' tensors concatenated along ``S`` are
        the one-shot run's ``block_current``); otherwise ``None``.  A stream in HBM -- four CUDA tensors as ``device_events``
        takes them -- is checked and staged where it lies (``nsof_accum_trials_step_dev``), with the same results bit for
        bit; the tensors may be freed when the call returns."""
        h = self._h
        dev = _device_stream("TrialAccumulator.step", self.ctx, x, y, p, t, bounds)
        if dev is None:
            x = np.ascontiguousarray(x, np.int16)
            y = np.ascontiguousarray(y, np.int16)
            p = np.ascontiguousarray(p, np.int8)
            t = np.ascontiguousarray(t, np.int64)
            bounds = np.ascontiguousarray(bounds, np.int64)
            if bounds.ndim != 1 or not (x.size == y.size == p.size == t.size):
                raise NsofValueError("event arrays of differing lengths")
            n = max(bounds.size - 1, 0)
            if n and (bounds[-1] > x.size or bounds[0] < 0):
                raise NsofValueError("event arrays shorter than the slice bounds")
        else:
            n = max(dev[-1], 0)
        cur = None
        if self.memsize is not None:
            s = int(self.ctx._lib.nsof_accum_trials_snaps_in(h, n))
            cur = self._empty((self.arrays, self.trials, s, self.H // self.memsize, self.W // self.memsize), _torch().float64)
        d_cur = dev_ptr(cur) if cur is not None and cur.numel() else None
        if n and dev is None:
            self.ctx.check(self.ctx._lib.nsof_accum_trials_step(h, x.ctypes.data, y.ctypes.data, p.ctypes.data, t.ctypes.data,
                                                                bounds.ctypes.data, n, d_cur, None), "accum_trials_step")
        elif n:
            self.ctx.check(self.ctx._lib.nsof_accum_trials_step_dev(h, *dev, d_cur, None), "accum_trials_step")
        return cur

    def w_dev(self):
        """The states, float32 CUDA tensor ``[A][T][H][W]`` (asynchronous on the context's stream, like every ``*_dev``)."""
        out = self._empty((self.arrays, self.trials, self.H, self.W), _torch().float32)
        self.ctx.check(self.ctx._lib.nsof_accum_trials_w_dev(self._h, dev_ptr(out)), "accum_trials_w")
        return out

    def resistance_dev(self):
        """``resistance_exp`` of the states, float32 CUDA tensor ``[A][T][H][W]``."""
        out = self._empty((self.arrays, self.trials, self.H, self.W), _torch().float32)
        self.ctx.check(self.ctx._lib.nsof_accum_trials_resistance_dev(self._h, dev_ptr(out)), "accum_trials_resistance")
        return out

    def block_current_dev(self):
        """The block maxima of ``v_ds / R`` of the CURRENT states, float64 CUDA tensor ``[A][T][H // memsize][W // memsize]``."""
        if self.memsize is None:
            raise NsofValueError("block currents need a memsize at creation")
        out = self._empty((self.arrays, self.trials, self.H // self.memsize, self.W // self.memsize), _torch().float64)
        self.ctx.check(self.ctx._lib.nsof_accum_trials_block_current_dev(self._h, dev_ptr(out)), "accum_trials_block_current")
        return out

    def _surface(self, fn, dtype, out, which, mode):
        torch = _torch()
        if mode not in ("current", "state"):
            raise NsofValueError("mode must be 'current' or 'state'")
        if out is None:
            out = self._empty((self.trials, self.H, self.W), dtype)
        if out.dtype != dtype or tuple(out.shape) != (self.trials, self.H, self.W) or out.stride(2) != 1 or not out.is_cuda:
            raise NsofValueError(f"the surfaces are a {dtype} CUDA tensor [{self.trials}][{self.H}][{self.W}] with pixel stride 1 "
                                 f"(got {out.dtype} {tuple(out.shape)}, strides {tuple(out.stride())})", _lib.NSOF_ESHAPE)
        size = out.element_size()
        self.ctx.check(fn(self._h, int(which), {"current": 0, "state": 1}[mode], dev_ptr(out), out.stride(1) * size,
                          (out.stride(0) if self.trials > 1 else self.H * out.stride(1)) * size), "accum_trials_surface")
        return out

    def surface_u8_dev(self, out=None, which=0, mode="state"):
        """The surfaces of array ``which`` of all trials as 8-bit frames, uint8 CUDA tensor ``[T][H][W]`` (``out``: such a
        tensor, rows and trials may be padded; ``None``: a new one) -- frame ``t`` is ``Accumulator.surface_u8`` of trial
        ``t``'s array, the frames ``farneback_sequence`` takes.  One launch; ``mode`` as there."""
        return self._surface(self.ctx._lib.nsof_accum_trials_surface_u8_dev, _torch().uint8, out, which, mode)

    def surface_f32_dev(self, out=None, which=0, mode="state"):
        """The same surfaces unquantised, float32 ``[T][H][W]`` (``Accumulator.surface_f32``)."""
        return self._surface(self.ctx._lib.nsof_accum_trials_surface_f32_dev, _torch().float32, out, which, mode)

    def state(self):
        """-> dict(w float32 [A][T][H][W], next_ok int64 [A][H][W], slice_counter): everything a resume needs."""
        w = np.empty((self.arrays, self.trials, self.H, self.W), np.float32)
        nok = np.empty((self.arrays, self.H, self.W), np.int64)
        cnt = C.c_int64()
        self.ctx.check(self.ctx._lib.nsof_accum_trials_read_state(self._h, w.ctypes.data, nok.ctypes.data, C.byref(cnt)),
                       "accum_trials_read_state")
        return dict(w=w, next_ok=nok, slice_counter=cnt.value)

    def load_state(self, state):
        """Inverse of ``state()``; ``next_ok`` may be missing (zeros), ``slice_counter`` too (0).  Shapes that do not match
        are refused before the library is called."""
        w = np.ascontiguousarray(state["w"], np.float32)
        if w.shape != (self.arrays, self.trials, self.H, self.W):
            raise NsofValueError(f"state['w'] is {w.shape}, the object holds {(self.arrays, self.trials, self.H, self.W)}", _lib.NSOF_ESHAPE)
        nok = state.get("next_ok")
        if nok is not None:
            nok = np.ascontiguousarray(nok, np.int64)
            if nok.shape != (self.arrays, self.H, self.W):
                raise NsofValueError(f"state['next_ok'] is {nok.shape}, the object holds {(self.arrays, self.H, self.W)}", _lib.NSOF_ESHAPE)
        cnt = state.get("slice_counter", 0)
        if isinstance(cnt, (bool, np.bool_)) or not isinstance(cnt, (int, np.integer)) or cnt < 0:
            raise NsofValueError(f"state['slice_counter'] = {cnt!r} is not a whole number >= 0")
        self.ctx.check(self.ctx._lib.nsof_accum_trials_write_state(self._h, w.ctypes.data, self.arrays * self.trials,
                                                                   None if nok is None else nok.ctypes.data, self.arrays, int(cnt)),
                       "accum_trials_write_state")

    def reset(self):
        """Back to the ``wini`` planes, zero refractory maps, slice counter 0."""
        self.ctx.check(self.ctx._lib.nsof_accum_trials_reset(self._h), "accum_trials_reset")

    def close(self):
        if getattr(self, "_p", None) is not None:
            self.ctx._lib.nsof_accum_trials_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def simulate_trials_dev(events, param_maps, version=1, slice_us=1_000, active_v=-8.0, silent_v=0.0, polarity="split", *,
                        sensor_size=None, params=None, dt=None, refractory_us=None, theta_events=None, snapshot_every=None,
                        memsize=None, v_ds=1.0, ctx=None, trials=None, c2c=None):
    """Monte-Carlo device trials of the event-driven accumulator in one run (``nsof_accum_trials_dev``): ``events`` as for
    ``simulate``, ``param_maps`` a mapping key of ``PARAMS`` -> ``[H][W]`` (shared by the trials) or ``[T][H][W]`` array read as
    float32 (``trial_param_maps_arg``; ``variability_maps(..., trials=T)`` draws them), the other arguments as for
    ``Accumulator``.  Returns a dict of CUDA tensors, ``A`` = 2 for ``version=2`` with ``polarity="split"``, else 1:
    ``w`` float32 [A][T][H][W] the final states, ``resistance`` float32 [A][T][H][W], and with ``memsize`` also
    ``block_current`` float64 [A][T][S][H // memsize][W // memsize] -- the block maxima of ``v_ds / R`` after the slices at
    which ``Accumulator.step(snap_every=snapshot_every)`` snapshots (``snapshot_every=None``: ``simulate``'s cadence,
    ``max(1, nslices // 100)``), what ``block_current_dev(memsize, snapshot=s)`` gives; ``block_current[0][t]`` is a gating
    stack.  Trial ``t`` equals ``Accumulator(param_maps=planes[t])`` stepped over the same stream bit for bit; the events are
    scattered and resolved once for all trials.  ``trials=T``: the number of trials where no plane says it (``param_maps``
    may then be ``None`` or ``{}``: identical devices); a ``[T'][H][W]`` plane with ``T' != T`` is refused.
    ``c2c``: cycle-to-cycle write noise (``c2c_arg``: ``dict(sigma=...)`` or ``dict(sigma_on=..., sigma_off=...)``, with
    ``seed``) -- every update ``w + g * dt`` becomes ``w + (g * f) * dt`` with ``f = max(0, 1 + sigma * xi)``, ``sigma`` that of
    the branch the drive took (``sigma_off``: ``V < voff``, ``sigma_on``: ``V > von``) and ``xi = c2c_noise(seed, a, t, y * W + x,
    slice, 1)``, a pure function of its arguments: results do not depend on ``snapshot_every`` or on how many trials run.
    ``None``, or both spreads 0, is the noiseless run bit for bit.  ``active_v`` / ``silent_v``: a number, or a sequence of ``T``
    numbers, one per trial (``TrialAccumulator``, which this function creates, steps once over the whole stream and closes).
    ``events`` may be a stream in HBM -- four CUDA tensors as ``device_events`` takes them: bounds, check and staging then
    run on the device (``slice_index_array``, ``TrialAccumulator.step``), ``sensor_size`` must be given (without it the call
    is refused before any device work), and the tensors may be freed when the call returns.
    Every refusal -- arguments, shapes, the value domain of every plane -- comes before any device work.  Synchronous."""
    early =_trial_scalars(version, polarity, params, dt, refractory_us, theta_events, c2c, trials)
    in_hbm = not isinstance(events, (str, Path)) and any(_is_cuda(v) for v in events)
    if isinstance(events, (str, Path)):
        x, y, p, t, H, W = load_events(Path(events))  # noqa: N806
    elif in_hbm:
        # a stream in HBM (device_events): the sensor is not inferred -- that would be a reduction and a wait of its own
        if sensor_size is None:
            raise NsofValueError("simulate_trials_dev: a device event stream needs sensor_size = (H, W)")
        x, y, p, t = events
        if device_events("simulate_trials_dev", x, y, p, t, ctx) == 0:
            raise NsofValueError("empty event stream")
        H, W = (int(v) for v in sensor_size)  # noqa: N806
    else:
        x, y, p, t = events
        x, y, t = np.asarray(x), np.asarray(y), np.asarray(t)
        if x.size == 0:
            raise NsofValueError("empty event stream")
        H, W = (int(y.max()) + 1, int(x.max()) + 1) if sensor_size is None else (int(v) for v in sensor_size)  # noqa: N806
    # (the cadence is checked here with a stand-in where it follows from the stream: that is known only below)
    cfg = _trial_config(early, H, W, param_maps, active_v, silent_v, trials, 1 if snapshot_every is None and memsize is not None else snapshot_every,
                        memsize, v_ds)
    if in_hbm:
        x16, y16, p8, t64 = x, y, p, t
        ctx = ctx or default_context()
    else:
        x16, y16 = np.ascontiguousarray(x, np.int16), np.ascontiguousarray(y, np.int16)
        p8, t64 = np.ascontiguousarray(p, np.int8), np.ascontiguousarray(t, np.int64)
        if not (x16.size == y16.size == p8.size == t64.size):
            raise NsofValueError("event arrays of differing lengths")
    idx = slice_index_array(t64, slice_us, ctx)
    nslices = len(idx) - 1
    if nslices < 1:
        raise NsofValueError("the event stream holds no slice")
    cfg["every"] = max(1, nslices // 100) if snapshot_every is None else int(snapshot_every)
    acc = TrialAccumulator(H, W, param_maps, ctx=ctx, _config=cfg)
    try:
        cur = acc.step(x16, y16, p8, t64, idx)
        out = dict(w=acc.w_dev(), resistance=acc.resistance_dev())
        if cur is not None:
            out["block_current"] = cur
        acc.ctx.synchronize()
    finally:
        acc.close()
    return out


def simulate_trials(events, param_maps, version=1, slice_us=1_000, active_v=-8.0, silent_v=0.0, polarity="split", **kw):
    """``simulate_trials_dev`` with the results downloaded: the same dict of NumPy arrays."""
    return {k: v.cpu().numpy() for k, v in simulate_trials_dev(events, param_maps, version, slice_us, active_v, silent_v, polarity,
                                                               **kw).items()}


def _frame_noise_args(trials, c2c, first_pair):
    """The scalar arguments the two frame-driven entries share, checked before the frames are looked at: ``(c2c_arg(c2c),
    int(first_pair))``.  Raises ``NsofValueError``, in this order, for what ``c2c_arg`` refuses, ``trials`` other than
    ``None`` or a whole number >= 1, and ``first_pair`` other than a whole number in ``[0, 2**63)``."""
    noise = c2c_arg(c2c)
    if trials is not None and (not isinstance(trials, (int, np.integer)) or isinstance(trials, (bool, np.bool_)) or trials < 1):
        raise NsofValueError(f"trials = {trials!r} is not a whole number >= 1")
    if isinstance(first_pair, (bool, np.bool_)) or not isinstance(first_pair, (int, np.integer)) or not 0 <= int(first_pair) < 2**63:
        raise NsofValueError(f"first_pair = {first_pair!r} is not a whole number >= 0 (a pair index)")
    return noise, int(first_pair)


def _frame_trial_maps(param_maps, shape, trials, noise):
    """``(n_trials, maps, AccumC2c or None)`` of a frame-driven call on ``shape`` = ``(H, W)`` frames: ``trials`` sets the trial
    count where no plane does.  Raises ``NsofValueError`` -- before a context exists -- for what ``frame_param_maps_arg``
    refuses, a ``[T'][H][W]`` plane with ``T' != trials`` (``NSOF_ESHAPE``) and noise with more than 65535 trials
    (``NSOF_EUNSUPPORTED``: the trial shares its counter word with the array)."""
    n_trials, maps = frame_param_maps_arg(param_maps, shape)
    if trials is not None:
        for k, a in maps:   # (a 2-D plane arrives here as [1][H][W]: shared by the trials)
            if np.ndim(param_maps[k]) == 3 and a.shape[0] != trials:
                raise NsofValueError(f"param_maps[{k!r}] holds {a.shape[0]} trials, trials = {trials}", _lib.NSOF_ESHAPE)
        n_trials = int(trials)
    if noise is not None and (np.float32(noise[1]) != 0 or np.float32(noise[2]) != 0) and n_trials > 65535:
        raise NsofValueError(f"c2c with {n_trials} trials: at most 65535 trials draw distinct variates", _lib.NSOF_EUNSUPPORTED)
    return n_trials, maps, None if noise is None else _lib.AccumC2c(*noise)


def simulate_frames(compressed_images, dt=0.0005, n_sub_steps=1000, th1=0.7, th2=1.5, *, ctx=None, params=None,
                    param_maps=None, trials=None, c2c=None, first_pair=0):
    """Frame-driven accumulator of /root/reference/simulation/simulationcode_v4_transistor_uav.m
    (``simulate_memristor_array``, :187-227): ``compressed_images`` float64 [n][H][W] in [0,1] (the output of the
    script's Lanczos ``compress_image``).  Returns ``(w_array, resistances_over_time)`` with the initial snapshot
    first, as the script stores them.  uav: th1=0.7, th2=1.5; vehicle: th1=2.  ``params``: the script's ``params`` struct as
    a mapping with the keys of ``PARAMS`` (``None``: ``PARAMS``), read as float64; ``dt`` is the argument it is.
    ``param_maps`` (a mapping key of ``PARAMS`` -> ``[H][W]`` or ``[T][H][W]`` array, ``frame_param_maps_arg``): a device per
    cell and per trial, all ``T`` trials in one launch; the other keys keep the scalar of
    ``params``.  Both results then gain a leading trial axis -- ``w [T][H][W]``, ``resistances [T][n][H][W]`` -- also for
    ``T`` = 1 (every plane 2-D); each (trial, cell) equals the uniform run at that cell's parameters bit for bit.  Either
    way it is one call of ``nsof_accum_frames_f64_c2c``: without maps, one trial whose axis is dropped (a view).
    ``trials=T``: the number of trials where no plane says it (``param_maps`` may then be ``None`` or ``{}``: identical
    devices); a ``[T'][H][W]`` plane with ``T' != T`` is refused.  The results carry the trial axis if and only if
    ``param_maps is not None or trials is not None``.
    ``c2c``: cycle-to-cycle write noise (``c2c_arg``: ``dict(sigma=...)`` or ``dict(sigma_on=..., sigma_off=...)``, with
    ``seed`` -- the event path's definition): per frame pair ``q = first_pair + f`` of trial ``t`` and cell ``i = r * W + c``
    one factor ``f = max(0, 1 + sigma * xi)`` with ``xi = c2c_noise(seed, 0, t, i, q, 1)`` and ``sigma`` that of the branch
    the pair's voltage takes at the cell's own thresholds (``sigma_off``: ``V < voff``, ``sigma_on``: ``V > von``, the dead
    zone: none), held for all ``n_sub_steps`` sub-steps: ``w + (dwdt * f) * dt / n_sub_steps``.  A pure function of its
    arguments: a trial's result does not depend on how many trials run.  ``None``, or both spreads 0, is the noiseless run
    bit for bit; ``c2c`` alone runs trial 0 and returns today's shapes.
    ``first_pair`` (a whole number >= 0): the index of the call's first pair -- a video can be run in chunks, frames
    ``[0:k + 1]`` and then ``[k:]`` with ``param_maps=dict(wini=w_of_the_first_call)`` and ``first_pair=k``, and gives the
    one-shot run's ``w`` and the matching slices of ``resistances`` bit for bit.  Without noise it has no effect.
    Every refusal -- ``c2c``, ``trials``, ``first_pair``, then the shapes -- comes before a context is created."""
    ap = accum_params(params)
    noise, first_pair = _frame_noise_args(trials, c2c, first_pair)
    imgs = np.ascontiguousarray(compressed_images, np.float64)
    if imgs.ndim != 3:
        raise NsofValueError("compressed_images must be [n][H][W]")
    n, H, W = imgs.shape  # noqa: N806
    n_trials, maps, nz = _frame_trial_maps(param_maps, (H, W), trials, noise)
    ctx = ctx or default_context()
    w = np.empty((n_trials, H, W), np.float64)
    res = np.empty((n_trials, n, H, W), np.float64)
    ctx.check(ctx._lib.nsof_accum_frames_f64_c2c(ctx.ptr, imgs.ctypes.data, n, H, W, float(dt), int(n_sub_steps), float(th1),
                                                 float(th2), C.byref(ap), n_trials, len(maps), *_frame_maps_c(n_trials, maps),
                                                 w.ctypes.data, res.ctypes.data, None if nz is None else C.byref(nz), first_pair),
              "simulate_frames")
    return (w, res) if param_maps is not None or trials is not None else (w[0], res[0])


def simulate_frames_dev(compressed, dt=0.0005, n_sub_steps=1000, th1=0.7, th2=1.5, v_ds=1.0, *, ctx=None, params=None,
                        param_maps=None, trials=None, c2c=None, first_pair=0):
    """``simulate_frames`` on a float64 CUDA tensor [n][H][W] (``frames.process_images_dev``'s output) in one launch
    (``nsof_accum_frames_f64_c2c_dev``, with or without maps or noise): returns ``(w [H][W], resistances [n][H][W], current [n-1][H][W])`` as float64 CUDA
    tensors -- ``w`` and ``resistances`` equal ``simulate_frames`` bit for bit, ``current[f] = v_ds / resistances[f + 1]``
    is the device current after pair (f, f+1), the layout ``gating.roi_from_surface_dev`` reads.  Nothing is copied;
    asynchronous on the context's stream.  ``params`` as for ``simulate_frames``.
    ``param_maps`` as for ``simulate_frames`` (host arrays; they are uploaded through a buffer of the context): every
    result gains a leading trial axis -- ``w [T][H][W]``, ``resistances [T][n][H][W]``, ``current [T][n-1][H][W]`` -- and
    ``current[t]`` is a gating stack of its own.
    ``trials``, ``c2c`` and ``first_pair`` as for ``simulate_frames``: the trial count where no plane says it, cycle-to-cycle
    write noise (one factor per frame pair) and the index of the call's first pair; the trial axis is there if and only if
    ``param_maps is not None or trials is not None``.  A chunked run -- frames ``[0:k + 1]``, then ``[k:]`` with
    ``param_maps=dict(wini=w.cpu().numpy())`` and ``first_pair=k`` -- equals the one-shot run in ``w``, ``resistances[..., k + 1:, :, :]``
    and ``current[..., k:, :, :]`` bit for bit."""
    ap = accum_params(params)
    noise, first_pair = _frame_noise_args(trials, c2c, first_pair)
    torch = _torch()
    if not isinstance(compressed, torch.Tensor) or not compressed.is_cuda:
        raise NsofValueError("simulate_frames_dev: a CUDA tensor expected", _lib.NSOF_EINVAL)
    if compressed.dtype != torch.float64:
        raise NsofValueError(f"simulate_frames_dev: float64 expected (got {compressed.dtype})", _lib.NSOF_EINVAL)
    if compressed.dim() != 3 or compressed.shape[0] < 1 or not compressed.is_contiguous():
        raise NsofValueError("simulate_frames_dev: contiguous [n][H][W] frames expected", _lib.NSOF_ESHAPE)
    n, H, W = (int(v) for v in compressed.shape)  # noqa: N806
    dev = compressed.device
    n_trials, maps, nz = _frame_trial_maps(param_maps, (H, W), trials, noise)
    ctx = ctx or default_context()
    w = torch.empty((n_trials, H, W), dtype=torch.float64, device=dev)
    res = torch.empty((n_trials, n, H, W), dtype=torch.float64, device=dev)
    cur = torch.empty((n_trials, n - 1, H, W), dtype=torch.float64, device=dev)
    ctx.check(ctx._lib.nsof_accum_frames_f64_c2c_dev(ctx.ptr, dev_ptr(compressed), n, H, W, float(dt), int(n_sub_steps),
                                                     float(th1), float(th2), float(v_ds), C.byref(ap), n_trials, len(maps),
                                                     *_frame_maps_c(n_trials, maps), dev_ptr(w), dev_ptr(res),
                                                     dev_ptr(cur) if n > 1 else None, None if nz is None else C.byref(nz),
                                                     first_pair), "simulate_frames_dev")
    return (w, res, cur) if param_maps is not None or trials is not None else (w[0], res[0], cur[0])


def _save_outputs(prefix, out, version, slice_us, polarity, h5_path, params=None, dt=None, refractory_us=None,
                  theta_events=None, param_maps=()):
    """File set of event_mem_sim.py:289-322 (npz keys ``w_final`` / ``resistances``; json.gz metadata).  The metadata holds
    the parameters, dt, refractory time and event threshold the run USED (the reference writes its module globals, which a dt overridden
    through ``update_state``'s default does not reach).  ``param_maps`` (``[(key, plane)]``): stored as ``map_<key>`` next to
    ``w_final`` and listed in the metadata; without maps neither file changes."""
    params = dict(PARAMS) if params is None else params
    dt = DT if dt is None else dt
    refractory_us = REFRACTORY_US if refractory_us is None else refractory_us
    theta_events = THETA_EVENTS if theta_events is None else theta_events
    np.savez_compressed(prefix.with_suffix(f".V{version}.npz"), w_final=out["w_final"],
                        resistances=out["resistances"].astype(np.float32), **{f"map_{k}": a for k, a in param_maps})
    if version == 2:
        if "w_final_b" in out:
            np.savez_compressed(prefix.with_suffix(".V2_b.npz"), w_final=out["w_final_b"],
                                resistances=out["resistances_b"].astype(np.float32))
        else:
            np.savez_compressed(prefix.with_suffix(".V2_b.npz"), w_final=np.array([]), resistances=np.array([]))
    meta = dict(version=version, slice_us=slice_us, fps=1_000_000 / slice_us, params=params, dt=dt,
                scheme="boxcar" if version == 1 else "dc_bias_overlay", polarity=polarity if version == 2 else None,
                theta_events=theta_events if version == 1 else None,
                refractory_us=refractory_us if version == 2 else None, event_file=str(h5_path or prefix))
    if param_maps:
        meta["param_maps"] = [k for k, _ in param_maps]
    with gzip.open(prefix.with_suffix(f".V{version}.json.gz"), "wt") as fp:
        json.dump(meta, fp, indent=2)
