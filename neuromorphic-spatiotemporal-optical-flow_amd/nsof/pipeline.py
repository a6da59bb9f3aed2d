"""Events -> temporal-prior surface -> ROI -> flow: the two stages chained (BASELINE.json configs 3 and 5).

The reference ships no code that connects the accumulator's output to the gating input (the
script that builds ``constructed3DMatrix`` is absent), so the glue here is build-defined and kept minimal:
    surface   resistance map R of the accumulator (``resistance_exp(w)``)
    current   I = V_ds / R with V_ds = 1 V (simulation/simulationcode_v4_transistor_uav.m:36)
    blocks    max of I over MEMSIZE x MEMSIZE pixel blocks  -> the coarse "memristor" map
    gating    ``current_to_gray`` -> threshold -> 4-connected components -> ROI  (nsof.gating, reference logic)
    flow      ``calcOpticalFlowFarneback`` on the ROI crop(s) of the frame pair
"""
import numpy as np

from . import gating
from .accumulator import Accumulator, slice_index_array
from .denoise import DENOISE_KEYS, events_denoise_dev, filter_args
from .events import events_from_frames_dev, events_from_video_dev, render_box_frames  # noqa: F401  (frames -> events, in HBM)
from .flowstats import events_flow_variability_dev  # noqa: F401  (the flow study of the event pipeline lives with its statistics)


def surface_to_block_current(resistance, memsize, v_ds=1.0):
    """Block-max of the device current over memsize x memsize pixel blocks (float64, [H//ms][W//ms])."""
    r = np.asarray(resistance, np.float64)
    hb, wb = r.shape[0] // memsize, r.shape[1] // memsize
    cur = v_ds / r[:hb * memsize, :wb * memsize]
    return cur.reshape(hb, memsize, wb, memsize).max(axis=(1, 3))


def events_to_rois(x, y, p, t, sensor_hw, cfg, version=1, polarity="split", slice_us=1000, active_v=-6.0,
                   silent_v=0.0, snapshot_every=33, ctx=None, max_rects=32, params=None, dt=None, refractory_us=None,
                   theta_events=None):
    """Run the accumulator over the stream and return, for every snapshot, the gating map and its ROI rectangles
    (x0, y0, x1, y1) in sensor pixels.  Everything between the event upload and the result stays in HBM: the block maxima of
    the device current of every snapshot (``Accumulator.block_current_dev``), then ONE gating call over all snapshots
    (``gating.roi_from_surface_dev``: gray map, threshold, connected components, rectangles -- for every map size); the
    rectangle table and the gray maps come back in one copy at the end.  With FLAG 2 a snapshot's list holds the union
    box alone (or nothing).  ``params`` / ``dt`` / ``refractory_us``: the accumulator's device model, ``theta_events``: scheme 1's event-count
    threshold (``Accumulator``)."""
    import torch

    from .context import default_context
    ctx = ctx or default_context()
    H, W = sensor_hw  # noqa: N806
    idx = slice_index_array(t, slice_us, ctx)
    rows, cols = H // cfg.MEMSIZE, W // cfg.MEMSIZE
    acc = Accumulator(H, W, version, polarity, active_v, silent_v, ctx=ctx, params=params, dt=dt, refractory_us=refractory_us,
                      theta_events=theta_events)
    try:
        acc.step(x, y, p, t, idx, snap_every=snapshot_every)
        n = acc.snapshot_count()
        if n == 0:
            return []
        cur = torch.empty((n, rows, cols), dtype=torch.float64, device=torch.device("cuda", ctx.device))
        for k in range(n):
            acc.block_current_dev(cfg.MEMSIZE, cur[k], snapshot=k)
        counts, rects, gray = gating.roi_from_surface_dev(cur, n, (rows, cols), (H, W), cfg, max_rects=max_rects, ctx=ctx,
                                                          want_gray=True)
        ctx.synchronize()
        most = int(counts.max().item())
        if most > max_rects:   # a map with more components than the table holds: one more (tiny) launch with room for all
            counts, rects, gray = gating.roi_from_surface_dev(cur, n, (rows, cols), (H, W), cfg, max_rects=most, ctx=ctx,
                                                              want_gray=True)
        lists = gating.rects_to_host(counts, rects, ctx=ctx)
        g = gray.cpu().numpy()
    finally:
        acc.close()
    return [(g[k], lists[k]) for k in range(n)]


def events_variability_dev(x, y, p, t, sensor_hw, cfg, rel_sigma, trials, seed=0, version=1, polarity="split", slice_us=1000,
                           active_v=-6.0, silent_v=0.0, snapshot_every=33, params=None, dt=None, refractory_us=None,
                           theta_events=None, max_rects=32, ctx=None, c2c=None):
    """What device-to-device variability does to the ROIs of an event stream, in HBM -- ``gating_variability_dev`` for the
    event pipeline.  The nominal array (``params``; ``None``: ``PARAMS``) is run as ``events_to_rois`` runs it (an
    ``Accumulator``, ``block_current_dev`` per snapshot); the ``trials`` arrays, whose pixels are drawn with the relative
    spreads ``rel_sigma`` (``variability_maps(H, W, rel_sigma, params, seed, trials=trials)``: trial ``t`` is seed
    ``seed + t``), take ONE trial run (``simulate_trials_dev``: the stream is scattered and resolved once for all of them).
    Then one launch of gate statistics (``gating.gate_stats_dev`` at ``cfg.THRES``) and one gating call over all
    ``trials * S`` maps of array 0 (``gating.roi_from_surface_dev``), ``S`` the number of snapshots.  Returns
    ``gating_variability_dev``'s dict of CUDA tensors: ``nominal`` float64 [S][rows][cols], ``stacks`` float64
    [T][S][rows][cols], ``counts`` int32 [S][rows][cols] and ``p_gate`` float64 (``counts / T``), ``flips`` int32 [T][S],
    ``rects`` int32 [T][S][max_rects][4] with ``rect_counts`` int32 [T][S].  An empty ``rel_sigma``, or a spread of 0 on every
    key, reproduces ``nominal`` in every trial bit for bit (a key whose spread is 0 keeps its scalar).  ``c2c``: cycle-to-cycle
    write noise on the trial arrays (``simulate_trials_dev``'s ``c2c``; the nominal array stays noiseless) -- the trial run is
    then always taken, with ``trials=trials``, also when ``rel_sigma`` is empty or all zero: identical devices that differ by
    their noise alone.  Synchronises at the end."""
    import torch

    from .accumulator import c2c_arg, simulate_trials_dev, variability_maps
    from .context import default_context
    from .errors import NsofValueError
    H, W = (int(v) for v in sensor_hw)  # noqa: N806
    variability_maps(1, 1, rel_sigma, params, seed, trials=trials)   # refuses before any device work
    c2c_arg(c2c)                                                      # ... and so does this
    for name, v in (("active_v", active_v), ("silent_v", silent_v)):
        if isinstance(v, (str, bytes)) or np.ndim(v) != 0:
            raise NsofValueError(f"events_variability_dev: {name} = {v!r} must be one number -- the nominal array has one operating "
                                 "point; a voltage per trial is TrialAccumulator's / simulate_trials_dev's")
    ctx = ctx or default_context()
    rows, cols = H // cfg.MEMSIZE, W // cfg.MEMSIZE
    acc = Accumulator(H, W, version, polarity, active_v, silent_v, ctx=ctx, params=params, dt=dt, refractory_us=refractory_us,
                      theta_events=theta_events)
    try:
        acc.step(x, y, p, t, slice_index_array(t, slice_us, ctx), snap_every=snapshot_every)
        n = acc.snapshot_count()
        nominal = torch.empty((n, rows, cols), dtype=torch.float64, device=torch.device("cuda", ctx.device))
        for k in range(n):
            acc.block_current_dev(cfg.MEMSIZE, nominal[k], snapshot=k)
        ctx.synchronize()
    finally:
        acc.close()
    # the planes of the keys that do vary (the draws of the others are made all the same: a key's plane does not depend on
    # which other spreads are zero)
    maps = {k: v for k, v in variability_maps(H, W, rel_sigma, params, seed, trials=trials).items() if float(rel_sigma[k]) != 0.0}
    if maps or c2c is not None:
        noisy = {} if c2c is None else dict(trials=int(trials), c2c=c2c)
        stacks = simulate_trials_dev((x, y, p, t), maps, version, slice_us, active_v, silent_v, polarity, sensor_size=(H, W),
                                     params=params, dt=dt, refractory_us=refractory_us, theta_events=theta_events,
                                     snapshot_every=snapshot_every, memsize=cfg.MEMSIZE, ctx=ctx, **noisy)["block_current"][0]
    else:
        stacks = nominal.unsqueeze(0).repeat(int(trials), 1, 1, 1)
    counts, flips = gating.gate_stats_dev(stacks, nominal, cfg.THRES, ctx=ctx)
    rect_counts, rects = gating.roi_from_surface_dev(stacks, int(trials) * n, (rows, cols), (H, W), cfg, max_rects=max_rects, ctx=ctx)
    ctx.synchronize()
    return dict(nominal=nominal, stacks=stacks, counts=counts, p_gate=counts.to(torch.float64) / int(trials), flips=flips,
                rects=rects.view(int(trials), n, max_rects, 4), rect_counts=rect_counts.view(int(trials), n))


def events_to_rois_host(x, y, p, t, sensor_hw, cfg, version=1, polarity="split", slice_us=1000, active_v=-6.0,
                        silent_v=0.0, snapshot_every=33, ctx=None, params=None, dt=None, refractory_us=None, theta_events=None):
    """The same through the host-side mirror of the reference's gating (``gating.connectedComponentsWithStats`` on the
    downloaded block currents): kept as the independent path the device kernel is tested against."""
    H, W = sensor_hw  # noqa: N806
    idx = slice_index_array(t, slice_us, ctx)
    acc = Accumulator(H, W, version, polarity, active_v, silent_v, ctx=ctx, params=params, dt=dt, refractory_us=refractory_us,
                      theta_events=theta_events)
    try:
        acc.step(x, y, p, t, idx, snap_every=snapshot_every)
        blocks = [acc.block_current(cfg.MEMSIZE, snapshot=k) for k in range(acc.snapshot_count())]
    finally:
        acc.close()
    out = []
    for cur in blocks:
        g = gating.current_to_gray(cur)
        tp = np.zeros((H // cfg.MEMSIZE, W // cfg.MEMSIZE))
        tp = gating.update_transition_pic(g, tp, cfg.THRES).astype(np.uint8)
        n, _, stats, _ = gating.connectedComponentsWithStats(tp, cfg.CONNECT)
        rects = [gating._roi(*[int(v) for v in stats[i, :4]], W, H, cfg.MEMSIZE, cfg.MEMSIZE, cfg) for i in range(1, n)]
        out.append((g, rects))
    return out


def events_to_roi_flows(x, y, p, t, sensor_hw, cfg, slice_us=1000, active_v=-6.0, silent_v=0.0, snapshot_every=33,
                        surface_mode="state", ctx=None, max_rects=32, timings=None, surface_dtype="uint8", params=None, dt=None,
                        refractory_us=None, theta_events=None):
    """BASELINE config 3 as one pipeline on the device: event stream -> leaky-integrate surface (scheme 1) -> every
    ``snapshot_every`` slices an 8-bit surface frame AND the gating map of the same state -> ROI rectangles on the device
    (``gating.roi_from_surface_dev``) -> Farneback flow of every ROI crop between consecutive surface frames, all crops of
    all pairs as ONE work list (``farneback_roi_sequence_dev``), written into frame-sized zero canvases exactly as
    ``opticalFlow3D`` pastes them (optical_flow_seg.py:129-164, 186-204; with FLAG 1 overlapping component boxes are pasted
    in label order, later ones winning).  Which map gates pair (k, k+1) follows ``cfg.bug_compatible`` like the host
    harness (``gating.gating_maps``): True (the default) = the map of frame k, as the shipped scripts do
    (``memimg2 := memimg1``, optical_flow_seg.py:435), False = the map of frame k+1, as ``opticalFlow3D`` is written.
    Events are uploaded once; frames, maps, rectangles and flow stay in HBM -- the only thing that crosses PCIe before the
    result is the rectangle table (16 bytes per ROI, one copy): the work list's shapes are needed on the host.
    Returns ``(frames uint8 [n][H][W], rects [[(x0, y0, x1, y1), ...] per frame], flows float32 [n-1][H][W][2])`` -- torch
    CUDA tensors and the host-side rectangle lists; ``flows[k]`` is zero outside the ROIs of the gating frame.
    ``surface_dtype="float32"``: the surface frames are the unquantised float surface instead (``Accumulator.run`` of the
    interval, then ``Accumulator.surface_f32``, same ``surface_mode``), ``frames`` is float32 and the crops run on
    ``farneback_roi_sequence_f32_dev``.  The gating maps and so the rectangles do not depend on it.
    ``params`` / ``dt`` / ``refractory_us``: the accumulator's device model, ``theta_events``: its event-count threshold
    (``Accumulator``)."""
    import time

    import torch

    from .context import default_context
    from .farneback import farneback_roi_sequence_dev, farneback_roi_sequence_f32_dev
    ctx = ctx or default_context()
    if surface_dtype not in ("uint8", "float32"):
        raise ValueError(f"surface_dtype must be 'uint8' or 'float32' (got {surface_dtype!r})")
    f32 = surface_dtype == "float32"
    H, W = sensor_hw  # noqa: N806
    dev = torch.device("cuda", ctx.device)
    idx = slice_index_array(t, slice_us, ctx)
    n_frames = (len(idx) - 1) // snapshot_every
    if n_frames < 2:
        raise ValueError("the stream is shorter than two snapshots")
    rows, cols = H // cfg.MEMSIZE, W // cfg.MEMSIZE
    frames = torch.empty((n_frames, H, W), dtype=torch.float32 if f32 else torch.uint8, device=dev)
    cur = torch.empty((n_frames, rows, cols), dtype=torch.float64, device=dev)
    flows = torch.empty((n_frames - 1, H, W, 2), dtype=torch.float32, device=dev)   # zero-filled by the flow call
    torch.cuda.synchronize(dev)
    acc = Accumulator(H, W, 1, "split", active_v, silent_v, ctx=ctx, params=params, dt=dt, refractory_us=refractory_us,
                      theta_events=theta_events)
    try:
        acc.set_events(x, y, p, t, idx)
        t0 = time.perf_counter()
        for k in range(n_frames):
            if f32:
                acc.run(k * snapshot_every, snapshot_every)
                acc.surface_f32(frames[k], mode=surface_mode)
            else:
                acc.run_surface(k * snapshot_every, snapshot_every, frames[k], mode=surface_mode)
            acc.block_current_dev(cfg.MEMSIZE, cur[k])
        counts, rtab = gating.roi_from_surface_dev(cur, n_frames, (rows, cols), (H, W), cfg, max_rects=max_rects, ctx=ctx)
        ctx.synchronize()
        most = int(counts.max().item())
        if most > max_rects:   # more components than the table holds: one more (tiny) gating launch with room for all
            counts, rtab = gating.roi_from_surface_dev(cur, n_frames, (rows, cols), (H, W), cfg, max_rects=most, ctx=ctx)
            ctx.synchronize()
        t1 = time.perf_counter()
        # crop -> flow -> paste of every ROI of every pair: one native call builds the work list from the rectangle table
        roi_flow = farneback_roi_sequence_f32_dev if f32 else farneback_roi_sequence_dev
        n_calls, n_pixels = roi_flow(frames, counts, rtab, flows, cfg.farneback_params,
                                     gate_frame=0 if cfg.bug_compatible else 1, ctx=ctx)
        ctx.synchronize()
        t2 = time.perf_counter()
        rects = gating.rects_to_host(counts, rtab, ctx=ctx)
    finally:
        acc.close()
    if timings is not None:
        timings.update(surface_and_gating_s=t1 - t0, flow_s=t2 - t1, frames=n_frames, roi_calls=int(n_calls), roi_pixels=int(n_pixels))
    return frames, rects, flows


def events_to_flow_sequence(x, y, p, t, sensor_hw, params=None, slice_us=1000, active_v=-6.0, silent_v=0.0,
                            snapshot_every=33, dense=None, ctx=None, timings=None, accum_params=None, dt=None,
                            refractory_us=None, theta_events=None):
    """BASELINE config 5 as one device-resident pipeline: event stream -> dense scheme-1 accumulator update of every
    slice -> every ``snapshot_every`` slices the surface as an 8-bit frame (``Accumulator.surface_u8``, mode "state":
    uint8(255 * w) -- the reference's current -> gray map saturates for the simulator's w >= 0.5 and the reference has
    no surface -> frame step of its own) -> Farneback flow between consecutive surface frames
    (``farneback_sequence``: every frame's pyramid and expansion computed once).  Events are uploaded once; frames and
    flow never leave HBM.  Returns ``(frames uint8 [n][H][W], flows float32 [n-1][H][W][2])`` as torch CUDA tensors.
    ``dense``: None (default) = the accumulator picks (with ``silent_v`` in the dead zone: frames as copy + patch of the
    previous one, ``nsof_accum_run_frames``), True = the every-pixel pass per interval (the roofline run), False = the
    event-pixel update.  Same frames either way.  ``timings`` (a dict) receives the wall time of the two stages.
    ``accum_params`` / ``dt`` / ``refractory_us``: the accumulator's device model, ``Accumulator``'s ``params`` / ``dt`` /
    ``refractory_us`` (``params`` is taken here: the Farneback parameters); ``theta_events``: its event-count threshold
    (above 1 the frames come from copy + patch, never the tile walk: same bytes)."""
    import time

    import torch

    from .context import default_context
    from .farneback import PARAMS_A, farneback_sequence
    ctx = ctx or default_context()
    params = params or PARAMS_A
    H, W = sensor_hw  # noqa: N806
    dev = torch.device("cuda", ctx.device)
    idx = slice_index_array(t, slice_us, ctx)
    n_slices = len(idx) - 1
    n_frames = n_slices // snapshot_every
    if n_frames < 2:
        raise ValueError("the stream is shorter than two snapshots")
    frames = torch.empty((n_frames, H, W), dtype=torch.uint8, device=dev)
    flows = torch.empty((n_frames - 1, H, W, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    acc = Accumulator(H, W, 1, "split", active_v, silent_v, ctx=ctx, dense=dense, params=accum_params, dt=dt,
                      refractory_us=refractory_us, theta_events=theta_events)
    try:
        acc.set_events(x, y, p, t, idx)
        t0 = time.perf_counter()
        acc.run_frames(0, n_frames, snapshot_every, frames)   # the frame of every interval from its last update pass
        ctx.synchronize()
        t1 = time.perf_counter()
        farneback_sequence(frames, flows, n_frames, H, W, params, ctx=ctx)
        ctx.synchronize()
        t2 = time.perf_counter()
    finally:
        acc.close()
    if timings is not None:
        timings.update(accumulator_s=t1 - t0, flow_s=t2 - t1, slices=n_frames * snapshot_every, frames=n_frames)
    return frames, flows


def video_to_flow_sequence(frames, times_us=None, *, frame_us=None, threshold=10.0, threshold_off=None, threshold_maps=None,
                           response=None, ref=None, timestamps="linear", p_on=1, p_off=-1, sensor=None, denoise=None, ctx=None,
                           **accumulator_args):
    """A grey video in HBM through the event pipeline: ``events_from_frames_dev(frames, ...)`` (the arguments up to
    ``p_off``) turns the frames into an event stream in HBM, and ``events_to_flow_sequence(x, y, p, t, (H, W),
    **accumulator_args)`` takes it where it lies -- slice bounds, check and staging on the device
    (``slice_index_array``, ``Accumulator.set_events``); only the bounds come to the host --, accumulates it and takes the
    flow between its surface frames.  Returns ``(surface frames uint8 [m][H][W], flows float32 [m-1][H][W][2],
    events)``, ``events`` the generator's result dict (``x, y, p, t`` CUDA tensors, ``frame_bounds``, ``ref``).  ``sensor``: a
    dict of the generator's sensor arguments (``refractory_us``, ``noise``, ``t_ok``, ``first_frame``), forwarded to it --
    apart from ``accumulator_args``, where ``refractory_us`` is the accumulator's; ``events`` then carries ``t_ok`` too.
    ``denoise``: a dict of the keyword arguments of ``events_denoise_dev`` (``dt_us``, and any of ``radius``, ``min_support``,
    ``same_polarity``, ``include_self``, ``last``): the background-activity filter is applied to the stream in HBM, between the
    generator and the accumulator, with the generator's ``frame_bounds`` as its bounds.  ``events`` then holds the kept stream
    (``x, y, p, t`` and its ``frame_bounds``) and gains ``keep`` (uint8 CUDA, one byte per generated event), ``n_kept`` and
    ``last``.  A bad key or value of the dict is refused before the generator runs.  ``None``: no filter."""
    from . import _lib
    from .context import default_context
    from .errors import NsofValueError
    sensor = {} if sensor is None else sensor
    if not isinstance(sensor, dict) or any(k not in ("refractory_us", "noise", "t_ok", "first_frame") for k in sensor):
        raise NsofValueError(f"video_to_flow_sequence: sensor = {sensor!r}; a dict of refractory_us, noise, t_ok, first_frame expected",
                             _lib.NSOF_EINVAL)
    if denoise is not None and (not isinstance(denoise, dict) or "dt_us" not in denoise or any(k not in DENOISE_KEYS for k in denoise)):
        raise NsofValueError(f"video_to_flow_sequence: denoise = {denoise!r}; a dict of dt_us and any of radius, min_support, "
                             "same_polarity, include_self, last expected", _lib.NSOF_EINVAL)
    if denoise is not None and getattr(frames, "ndim", 0) == 3:   # (frames of another kind: the generator's refusal, below)
        # the filter's values too are refused here, before the generator has done any device work
        filter_args("video_to_flow_sequence: denoise", (int(frames.shape[1]), int(frames.shape[2])), **denoise)
        last = denoise.get("last")
        if last is not None and last.device != frames.device:
            raise NsofValueError("video_to_flow_sequence: denoise: last must be a CUDA tensor on the frames' device", _lib.NSOF_EINVAL)
    # (the generator refuses its arguments before it asks for a context; the default one is process-wide)
    ev = events_from_frames_dev(frames, times_us, frame_us=frame_us, threshold=threshold, threshold_off=threshold_off,
                                threshold_maps=threshold_maps, response=response, ref=ref, timestamps=timestamps, p_on=p_on,
                                p_off=p_off, ctx=ctx, **sensor)
    ctx = ctx or default_context()
    if denoise is not None:
        kept = events_denoise_dev(ev["x"], ev["y"], ev["p"], ev["t"], (int(frames.shape[1]), int(frames.shape[2])),
                                  bounds=ev["frame_bounds"], ctx=ctx, **denoise)
        ev = dict(ev, frame_bounds=kept.pop("bounds"), **kept)
    ctx.synchronize()
    surfaces, flows = events_to_flow_sequence(ev["x"], ev["y"], ev["p"], ev["t"], (int(frames.shape[1]), int(frames.shape[2])), ctx=ctx,
                                              **accumulator_args)
    return surfaces, flows, ev


def events_to_flow_sequence_sharded(x, y, p, t, sensor_hw, params=None, slice_us=1000, active_v=-6.0, silent_v=0.0,
                                    snapshot_every=33, dense=None, ctx=None, stats=None, accum_params=None, dt=None,
                                    refractory_us=None, theta_events=None):
    """``events_to_flow_sequence`` over the ranks of the current process group (one GPU each): accumulator row bands,
    all-gather of the 8-bit surface frames, contiguous shards of the frame pairs (``nsof.dist.events_to_flow_sharded``
    with the GPU accumulator and ``farneback_sequence`` as the two stages).  Returns ``((lo, hi), frames, flows_local)``
    -- torch CUDA tensors; ``flows_local`` are pairs ``lo .. hi-1`` of the sequence (None for a rank without pairs).
    ``accum_params`` / ``dt`` / ``refractory_us`` / ``theta_events`` as for ``events_to_flow_sequence``."""
    import torch

    from . import dist as nd
    from .context import default_context
    from .farneback import PARAMS_A, farneback_sequence
    ctx = ctx or default_context()
    params = params or PARAMS_A
    H, W = sensor_hw  # noqa: N806
    dev = torch.device("cuda", ctx.device)

    def band_frames(xb, yb, pb, tb, idx, hw, every, n_frames):
        rows, w = hw
        out = torch.empty((n_frames, rows, w), dtype=torch.uint8, device=dev)
        if rows == 0:
            return out
        acc = Accumulator(rows, w, 1, "split", active_v, silent_v, ctx=ctx, dense=dense, params=accum_params, dt=dt,
                          refractory_us=refractory_us, theta_events=theta_events)
        try:
            acc.set_events(xb, yb, pb, tb, idx)
            acc.run_frames(0, n_frames, every, out)
            ctx.synchronize()
        finally:
            acc.close()
        return out

    def flow_of_frames(fr):
        fr = fr.to(dev).contiguous()
        flows = torch.empty((fr.shape[0] - 1, H, W, 2), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        farneback_sequence(fr, flows, fr.shape[0], H, W, params, ctx=ctx)
        ctx.synchronize()
        return flows

    return nd.events_to_flow_sharded(x, y, p, t, (H, W), slice_us, snapshot_every, band_frames, flow_of_frames, device=dev
                                     if torch.distributed.is_initialized() and torch.distributed.get_backend() == "nccl"
                                     else None, stats=stats)


def gated_flow(gray_map, prev, nxt, cfg, flow_fn=None):
    """Flow of a frame pair restricted to the ROI(s) the gating map selects (``opticalFlow3D`` of the reference)."""
    kw = {} if flow_fn is None else {"flow_fn": flow_fn}
    return gating.opticalFlow3D(gray_map, gray_map, prev, nxt, cfg.MEMSIZE, cfg.MEMSIZE, cfg, **kw)


# ---- the segmentation experiment of optical_flow_seg.py (__main__, :399-632) as a function --------------------------
SEG_CSV_COLUMNS = ["Frame_Pair", "Original_Flow_Time", "Mem_Flow_Time", "Flow_Time_Improvement",
                   "Flow_Time_Improvement_Percent", "Original_Seg_Time", "Mem_Seg_Time", "Combination_Time",
                   "Original_PA", "Mem_PA", "Region_Percent", "Cal_Times", "Velocity_Times"]   # seg.py:365-379


def calculate_pixel_accuracy(image1, image2):
    """seg.py:383-387: share of identical pixels, in percent."""
    return float(np.sum(image1 == image2)) / image1.size * 100


def run_segmentation(frames_bgr, gt_masks_bgr, mem_state, cfg, names=None, csv_path=None, seg_th=1, merge_flag=False,
                     flow_fn=None, mask_fn=None):
    """The main loop of optical_flow_seg.py for a sequence held in memory: for every pair (i, i+1), i < n-2, the gated
    flow + segmentation ("Mem") and the full-frame flow + segmentation ("Original"), their times, their pixel
    accuracies against the ground-truth mask of frame i+1, and the CSV row the script writes (same 13 columns, same
    formatting).  ``frames_bgr`` / ``gt_masks_bgr``: uint8 [H][W][3] as ``cv2.imread`` returns them; ``mem_state``: the
    ``constructed3DMatrix`` stack.  ``flow_fn`` / ``mask_fn`` default to the GPU path (``calcOpticalFlowFarneback``,
    ``segment.motion_mask``); tests inject the CPU oracle.  Returns ``(rows, mean_mem_accuracy, mean_original_accuracy)``."""
    import csv
    import time

    from . import segment
    from .farneback import calcOpticalFlowFarneback
    flow_fn = flow_fn or calcOpticalFlowFarneback
    mask_fn = mask_fn or (lambda f: segment.motion_mask(f, seg_th))
    names = names or [f"{i + 1}.jpg" for i in range(len(frames_bgr))]
    rows, acc_mem, acc_orig = [], 0.0, 0.0
    if csv_path:
        with open(csv_path, "w", newline="") as fh:
            csv.writer(fh).writerow(SEG_CSV_COLUMNS)
    for i in range(len(frames_bgr) - 2):
        cfg.mem_opticalflow_times.clear(); cfg.mem_cal_times.clear(); cfg.mem_velocity_times.clear()
        memimg1, memimg2 = gating.gating_maps(mem_state, i, cfg)
        prev_gray = gating.frame_to_gray(frames_bgr[i], "RGB2GRAY")
        next_gray = gating.frame_to_gray(frames_bgr[i + 1], "RGB2GRAY")
        gt = np.where(gating.frame_to_gray(gt_masks_bgr[i + 1], "BGR2GRAY") > 127, np.uint8(255), np.uint8(0))
        h, w = next_gray.shape
        out = gating.opticalFlow3D(memimg1, memimg2, prev_gray, next_gray, cfg.MEMSIZE, cfg.MEMSIZE, cfg,
                                   flow_fn=flow_fn)
        flow, region_list = -out[0], out[3]
        if cfg.FLAG == 1:
            num_labels, regions = out[4], out[5]
        else:
            regions = out[4]
            num_labels = 2 if tuple(regions) != (0, 0, 0, 0) else 1
        # Mem segmentation (task_results, seg.py:253-320)
        t0 = time.time()
        motion = np.zeros((h, w), np.uint8)
        t_comb = 0.0
        if num_labels > 1:
            if cfg.FLAG == 1 and merge_flag:
                pad = 20
                boxes = [(max(0, min(r[0] for r in regions) - pad), max(0, min(r[1] for r in regions) - pad),
                          min(w, max(r[2] for r in regions) + pad), min(h, max(r[3] for r in regions) + pad))]
            else:
                boxes = list(regions) if cfg.FLAG == 1 else [tuple(regions)]
            t_comb = time.time() - t0
            for x0, y0, x1, y1 in boxes:
                if x1 > x0 and y1 > y0:
                    motion[y0:y1, x0:x1] = mask_fn(np.ascontiguousarray(flow[y0:y1, x0:x1], np.float32))
        t_mem_seg = time.time() - t0
        # Original: full-frame flow and segmentation (seg.py:493-537)
        t0 = time.time()
        flow1 = -flow_fn(prev_gray, next_gray, None, **cfg.farneback_params.as_kwargs())
        t_orig_flow = time.time() - t0
        t0 = time.time()
        motion1 = mask_fn(np.ascontiguousarray(flow1, np.float32))
        t_orig_seg = time.time() - t0
        a_mem, a_orig = calculate_pixel_accuracy(motion, gt), calculate_pixel_accuracy(motion1, gt)
        acc_mem += a_mem
        acc_orig += a_orig
        t_mem_flow = cfg.mem_opticalflow_times[0]
        imp = t_orig_flow - t_mem_flow
        row = [f"{names[i + 1]}-{names[i]}", f"{t_orig_flow:.4f}", f"{t_mem_flow:.4f}", f"{imp:.4f}",
               f"{imp / t_orig_flow * 100:.2f}", f"{t_orig_seg:.4f}", f"{t_mem_seg:.4f}", f"{t_comb:.4f}",
               f"{a_orig:.4f}", f"{a_mem:.4f}", region_list, ";".join(f"{t:.4f}" for t in cfg.mem_cal_times),
               ";".join(f"{t:.4f}" for t in cfg.mem_velocity_times)]
        rows.append(row)
        if csv_path:
            with open(csv_path, "a", newline="") as fh:
                csv.writer(fh).writerow(row)
    n = max(len(rows), 1)
    return rows, acc_mem / n, acc_orig / n


# ---- the prediction experiment of optical_flow_prediction.py (__main__, :435-681) as a function ---------------------
PREDICT_CSV_COLUMNS = ["Frame_Pair", "Original_Flow_Time", "Mem_Flow_Time", "Flow_Time_Improvement",
                       "Flow_Time_Improvement_Percent", "Original_Pred_Time", "Mem_Pred_Time", "Combination_Time",
                       "Original_SSIM", "Mem_SSIM", "Region_Percent", "Cal_Times", "Velocity_Times"]   # prediction.py:413-427
PREDICT_PADDING = 20   # prediction.py PADDING: the merged box of FLAG 1 with MERGE_FLAG


def prediction_boxes(regions, num_labels, flag, merge_flag, frame_hw, padding=PREDICT_PADDING):
    """The boxes the prediction task warps for one pair (prediction.py:268-353): none without a component, the union box
    (FLAG 2), every component box (FLAG 1), or their bounding box padded and clipped to the frame (FLAG 1 merged)."""
    h, w = frame_hw
    if num_labels <= 1:
        return []
    if flag != 1:
        return [tuple(regions)]
    if not merge_flag:
        return [tuple(r) for r in regions]
    return [(max(0, min(r[0] for r in regions) - padding), max(0, min(r[1] for r in regions) - padding),
             min(w, max(r[2] for r in regions) + padding), min(h, max(r[3] for r in regions) + padding))]


def run_prediction(frames_bgr, mem_state, cfg, names=None, csv_path=None, merge_flag=True, flow_fn=None, predict_fn=None,
                   ssim_fn=None):
    """The main loop of optical_flow_prediction.py for a sequence held in memory: for every pair (i, i+1), i < n-2, the
    gated flow + prediction ("Mem", ``task_results`` with MERGE_FLAG = ``merge_flag``; the script passes True) and the
    full-frame flow + prediction ("Original", BORDER_CONSTANT), their times, their SSIMs against frame i+2 (channel 2,
    ``calculateIntegralError``) and the CSV row the script writes (same 13 columns, same formatting).  ``frames_bgr``:
    uint8 [H][W][3] as ``cv2.imread`` returns them; ``mem_state``: the ``constructed3DMatrix`` stack.  ``flow_fn`` /
    ``predict_fn`` / ``ssim_fn`` default to the GPU path (``calcOpticalFlowFarneback``, ``predict.task_results``,
    ``predict.calculateIntegralError``); tests inject the CPU oracle.  ``predict_fn`` takes ``task_results``' arguments
    (``times`` / ``comb_times`` / ``borderMode`` keywords included).  Returns ``(rows, ssim_mem, ssim_orig,
    mean_mem_as_printed, mean_orig_as_printed)``: the per-pair SSIM lists and the means the script prints, which divide by
    ``cnt - 1`` (prediction.py:678; None for a single pair)."""
    import csv
    import time

    from . import predict
    from .farneback import calcOpticalFlowFarneback
    flow_fn = flow_fn or calcOpticalFlowFarneback
    predict_fn = predict_fn or predict.task_results
    ssim_fn = ssim_fn or predict.calculateIntegralError
    names = names or [f"{i + 1}.jpg" for i in range(len(frames_bgr))]
    rows, ssim_mem, ssim_orig = [], [], []
    if csv_path:
        with open(csv_path, "w", newline="") as fh:
            csv.writer(fh).writerow(PREDICT_CSV_COLUMNS)
    for i in range(len(frames_bgr) - 2):
        cfg.mem_opticalflow_times.clear(); cfg.mem_cal_times.clear(); cfg.mem_velocity_times.clear()
        memimg1, memimg2 = gating.gating_maps(mem_state, i, cfg)
        prev_frame, next_frame = frames_bgr[i], frames_bgr[i + 1]
        prev_gray = gating.frame_to_gray(prev_frame, "RGB2GRAY")
        next_gray = gating.frame_to_gray(next_frame, "RGB2GRAY")
        h, w = next_frame.shape[:2]
        out = gating.opticalFlow3D(memimg1, memimg2, prev_gray, next_gray, cfg.MEMSIZE, cfg.MEMSIZE, cfg,
                                   flow_fn=flow_fn)
        flow, region_list = (-out[0]).astype(np.float32), out[3]
        if cfg.FLAG == 1:
            num_labels, regions = out[4], out[5]
        else:
            regions = out[4]
            num_labels = 2 if tuple(regions) != (0, 0, 0, 0) else 1
        mem_times, comb_times = [], []
        pred = predict_fn(prev_frame, next_frame, flow, num_labels, regions, EST_FLAG=cfg.FLAG, MERGE_FLAG=merge_flag,
                          times=mem_times, comb_times=comb_times)
        s_mem = ssim_fn(pred, frames_bgr[i + 2])
        # Original: full-frame flow and prediction (prediction.py:566-605)
        t0 = time.time()
        flow1 = flow_fn(prev_gray, next_gray, None, **cfg.farneback_params.as_kwargs())
        t_orig_flow = time.time() - t0
        flow1 = -flow1
        t0 = time.time()
        pred1 = predict_fn(prev_frame, next_frame, flow1.astype(np.float32), 2, (0, 0, w, h), EST_FLAG=2,
                           MERGE_FLAG=False, borderMode=predict.BORDER_CONSTANT)
        t_orig_pred = time.time() - t0
        s_orig = ssim_fn(pred1, frames_bgr[i + 2])
        ssim_mem.append(s_mem)
        ssim_orig.append(s_orig)
        t_mem_flow = cfg.mem_opticalflow_times[0]
        imp = t_orig_flow - t_mem_flow
        row = [f"{names[i + 1]}-{names[i]}", f"{t_orig_flow:.4f}", f"{t_mem_flow:.4f}", f"{imp:.4f}",
               f"{imp / t_orig_flow * 100 if t_orig_flow else float('nan'):.2f}", f"{t_orig_pred:.4f}",
               f"{mem_times[0]:.4f}", f"{comb_times[0]:.4f}", f"{s_orig:.4f}", f"{s_mem:.4f}", region_list,
               ";".join(f"{t:.4f}" for t in cfg.mem_cal_times), ";".join(f"{t:.4f}" for t in cfg.mem_velocity_times)]
        rows.append(row)
        if csv_path:
            with open(csv_path, "a", newline="") as fh:
                csv.writer(fh).writerow(row)
    cnt = len(rows)
    mean_mem = sum(ssim_mem) / (cnt - 1) if cnt > 1 else None
    mean_orig = sum(ssim_orig) / (cnt - 1) if cnt > 1 else None
    return rows, ssim_mem, ssim_orig, mean_mem, mean_orig


def _sequence_flows(frames_bgr, mem_state, cfg, with_original, max_rects, ctx, what):
    """The front half of the sequence experiments in HBM: checks, gray frames (``gray_u8_dev``, RGB2GRAY as the scripts
    convert), the gating slices (a host ``(rows, cols, T)`` stack goes up; a float64 CUDA tensor [T][rows][cols], e.g.
    ``gating_stack_from_frames_dev``'s, is sliced where it is), the device gating table of slices OFFSET .. OFFSET+n-2 (one launch, ``gating.roi_from_surface_dev``;
    regrown once when a map has more than ``max_rects`` components), the ROI flows of pairs 0 .. n-3 from that table
    (``farneback_roi_sequence_dev``, gated as ``cfg.bug_compatible`` says) and, with ``with_original``, the full-frame
    flows (``farneback_sequence``).  Returns ``(gray, counts, rtab, rects, flow_mem, flow_orig, gate_frame)``: the gray
    frames (still being read by the flow calls: the caller holds them until it synchronises), the device table, the
    host rectangle lists of every pair and the un-negated flows (``flow_orig`` None without the original)."""
    import torch

    from . import predict
    from .farneback import farneback_roi_sequence_dev, farneback_sequence
    predict._u8_frames(frames_bgr, what)
    if frames_bgr.dim() != 4 or frames_bgr.shape[3] != 3:
        raise predict.NsofValueError(f"{what}: uint8 [n][H][W][3] frames expected")
    n, H, W = (int(v) for v in frames_bgr.shape[:3])  # noqa: N806
    if n < 3:
        raise ValueError(f"{what}: {n} frames; the experiment needs at least 3")
    on_device = isinstance(mem_state, torch.Tensor)   # [T][rows][cols] in HBM; a host stack is (rows, cols, T)
    if on_device and (not mem_state.is_cuda or mem_state.device != frames_bgr.device or mem_state.dtype != torch.float64
                      or mem_state.dim() != 3 or not mem_state.is_contiguous()):
        raise predict.NsofValueError(f"{what}: a gating stack given as a tensor must be a contiguous float64 "
                                     f"[T][rows][cols] tensor on {frames_bgr.device}")
    rows, cols, slices = (int(mem_state.shape[i]) for i in ((1, 2, 0) if on_device else (0, 1, 2)))
    if rows > H // cfg.MEMSIZE or cols > W // cfg.MEMSIZE:
        raise ValueError(f"gating map {rows}x{cols} larger than the {H // cfg.MEMSIZE}x{W // cfg.MEMSIZE} transition picture")
    if slices < cfg.OFFSET + n - 1:
        raise ValueError(f"the stack has {slices} slices; {n} frames need OFFSET + {n - 1}")
    gf = 0 if cfg.bug_compatible else 1
    dev = frames_bgr.device
    if on_device:
        cur = mem_state[cfg.OFFSET:cfg.OFFSET + n - 1]   # a view: the slices are read where they are
    else:
        cur = torch.from_numpy(np.ascontiguousarray(np.moveaxis(np.asarray(mem_state)[:, :, cfg.OFFSET:cfg.OFFSET + n - 1], 2, 0),
                                                    np.float64)).to(dev)
    gray = torch.empty((n - 1, H, W), dtype=torch.uint8, device=dev)
    flow_mem = torch.empty((n - 2, H, W, 2), dtype=torch.float32, device=dev)   # zero-filled by the ROI flow call
    flow_orig = torch.empty_like(flow_mem) if with_original else None
    torch.cuda.synchronize(dev)
    for k in range(n - 1):
        predict.gray_u8_dev(frames_bgr[k], gray[k], "RGB2GRAY", ctx=ctx)
    counts, rtab = gating.roi_from_surface_dev(cur, n - 1, (rows, cols), (H, W), cfg, max_rects=max_rects, ctx=ctx)
    ctx.synchronize()
    c, r = counts.cpu().numpy(), rtab.cpu().numpy()
    if c.max() > max_rects:   # more components than the table holds: one more (tiny) gating launch with room for all
        counts, rtab = gating.roi_from_surface_dev(cur, n - 1, (rows, cols), (H, W), cfg, max_rects=int(c.max()), ctx=ctx)
        ctx.synchronize()
        c, r = counts.cpu().numpy(), rtab.cpu().numpy()
    lists = [[tuple(int(v) for v in r[k, i]) for i in range(int(c[k]))] for k in range(n - 1)]
    farneback_roi_sequence_dev(gray, counts, rtab, flow_mem, cfg.farneback_params, gate_frame=gf, ctx=ctx)
    if with_original:
        farneback_sequence(gray, flow_orig, n - 1, H, W, cfg.farneback_params, row_stride=int(gray.stride(1)),
                           frame_stride=int(gray.stride(0)), ctx=ctx)
    rects = [lists[k + gf] for k in range(n - 2)]
    return gray, counts, rtab, rects, flow_mem, flow_orig, gf


def _compressed_grids_dev(frames_bgr, cfg, m, n, region, ctx, who):
    """The front half of the frame-driven gating path: BGR frames -> gray frames (``gray_u8_dev``, RGB2GRAY) -> Lanczos-3
    grids of ``region`` (``frames.process_images_dev``), float64 CUDA tensor [k][rows][cols]."""
    import torch

    from . import frames as fr
    from . import predict
    predict._u8_frames(frames_bgr, who)
    if frames_bgr.dim() != 4 or frames_bgr.shape[3] != 3 or frames_bgr.shape[0] < 2:
        raise predict.NsofValueError(f"{who}: at least two uint8 [k][H][W][3] frames expected")
    k, H, W = (int(v) for v in frames_bgr.shape[:3])  # noqa: N806
    gray = torch.empty((k, H, W), dtype=torch.uint8, device=frames_bgr.device)
    torch.cuda.synchronize(frames_bgr.device)
    for i in range(k):
        predict.gray_u8_dev(frames_bgr[i], gray[i], "RGB2GRAY", ctx=ctx)
    ul, lr = region if region is not None else (None, None)
    return fr.process_images_dev(gray, cfg.MEMSIZE if m is None else m, cfg.MEMSIZE if n is None else n, ul, lr, ctx=ctx)


def gating_stack_from_frames_dev(frames_bgr, cfg, m=None, n=None, region=None, ctx=None, **sim):
    """The gating stack of a video, simulated in HBM: ``frames_bgr`` uint8 CUDA tensor [k][H][W][3] (BGR as ``cv2.imread``
    gives them) -> gray frames (``gray_u8_dev``, the RGB2GRAY the flow stage converts with) -> Lanczos-3 grids of
    ``region`` (``(region_ul, region_lr)``, MATLAB corners; the whole frame by default) compressed by ``m`` columns and ``n``
    rows per cell (``frames.process_images_dev``; both default to ``cfg.MEMSIZE``, so the grid is the transition picture)
    -> the array run over all pairs in one launch (``simulate_frames_dev``; ``sim`` passes ``dt``, ``n_sub_steps``,
    ``th1``, ``th2``, ``v_ds``, ``params``, ``param_maps`` on).  Returns the device currents, float64 CUDA tensor
    [k-1][rows][cols]: slice f is the array after pair (f, f+1) -- what ``prediction_sequence_dev`` /
    ``segmentation_sequence_dev`` take as ``mem_state`` without a copy.  With ``param_maps=`` (a device per cell and per
    trial, ``simulate_frames_dev``) or ``trials=`` the result is [T][k-1][rows][cols], one such stack per trial.  ``sim`` also
    passes ``trials`` (the trial count where no plane says it), ``c2c`` (cycle-to-cycle write noise, one factor per frame
    pair) and ``first_pair`` (the index of the first pair, for a video run in chunks through ``wini``) on.  Without noise equal to
    ``frames.process_images`` -> ``simulate_frames`` -> ``v_ds / resistances[1:]`` on the host gray frames, bit for bit.
    Nothing visits the host; synchronises at the end (the intermediates are released)."""
    from .accumulator import simulate_frames_dev
    from .context import default_context
    ctx = ctx or default_context()
    grids = _compressed_grids_dev(frames_bgr, cfg, m, n, region, ctx, "gating_stack_from_frames_dev")
    cur = simulate_frames_dev(grids, ctx=ctx, **sim)[2]
    ctx.synchronize()
    return cur


def gating_variability_dev(frames_bgr, cfg, rel_sigma, trials, seed=0, params=None, max_rects=32, m=None, n=None, region=None,
                           ctx=None, c2c=None, **sim):
    """What device-to-device variability does to the gate of a sequence, in HBM: the frames are compressed once
    (``gating_stack_from_frames_dev``'s front half), the array is run for the nominal device ``params`` (``None``:
    ``PARAMS``) and for ``trials`` arrays whose cells are drawn with the relative spreads ``rel_sigma`` (``{key: sigma}``;
    ``variability_maps(rows, cols, rel_sigma, params, seed, trials=trials, dtype=float64)``: trial ``t`` is seed ``seed + t``)
    -- one launch each --, then one launch of gate statistics (``gating.gate_stats_dev`` at ``cfg.THRES``) and one gating call
    over all ``trials * (k - 1)`` maps (``gating.roi_from_surface_dev``).  ``sim`` passes ``dt``, ``n_sub_steps``, ``th1``,
    ``th2``, ``v_ds`` on.  Returns a dict of CUDA tensors: ``nominal`` float64 [k-1][rows][cols], ``stacks`` float64
    [T][k-1][rows][cols] (``stacks[t]`` is a ``mem_state`` of the sequence experiments, no copy), ``counts`` int32
    [k-1][rows][cols] and ``p_gate`` float64 (``counts / T``: the gate probability per cell), ``flips`` int32 [T][k-1]
    (cells of trial t's map f gated differently from the nominal's), ``rects`` int32 [T][k-1][max_rects][4] with
    ``rect_counts`` int32 [T][k-1] (the tables of ``roi_from_surface_dev`` per map).  A spread of 0 on every key reproduces
    ``nominal`` in every trial bit for bit.  ``c2c``: cycle-to-cycle write noise on the trial arrays (``simulate_frames_dev``'s
    ``c2c``: one factor per frame pair; the nominal array stays noiseless) -- the trial run is then always taken, with
    ``trials=trials``, also when ``rel_sigma`` is empty: identical devices that differ by their noise alone.  Synchronises at
    the end."""
    import numpy as np
    import torch

    from .accumulator import c2c_arg, simulate_frames_dev, variability_maps
    from .context import default_context
    maps = variability_maps(1, 1, rel_sigma, params, seed, trials=trials, dtype=np.float64)   # refuses before any device work
    c2c_arg(c2c)                                                                              # ... and so does this
    ctx = ctx or default_context()
    grids = _compressed_grids_dev(frames_bgr, cfg, m, n, region, ctx, "gating_variability_dev")
    k, rows, cols = (int(v) for v in grids.shape)
    H, W = (int(v) for v in frames_bgr.shape[1:3])  # noqa: N806
    nominal = simulate_frames_dev(grids, ctx=ctx, params=params, **sim)[2]
    if maps or c2c is not None:
        maps = variability_maps(rows, cols, rel_sigma, params, seed, trials=trials, dtype=np.float64) if maps else None
        noisy = {} if c2c is None else dict(trials=int(trials), c2c=c2c)
        stacks = simulate_frames_dev(grids, ctx=ctx, params=params, param_maps=maps, **noisy, **sim)[2]
    else:
        ctx.synchronize()                                # torch copies on its own stream: the nominal run must have finished
        stacks = nominal.unsqueeze(0).repeat(int(trials), 1, 1, 1)
        torch.cuda.synchronize(nominal.device)           # ... and the copy, before the context's stream reads it
    counts, flips = gating.gate_stats_dev(stacks, nominal, cfg.THRES, ctx=ctx)
    rect_counts, rects = gating.roi_from_surface_dev(stacks, int(trials) * (k - 1), (rows, cols), (H, W), cfg, max_rects=max_rects,
                                                     ctx=ctx)
    ctx.synchronize()
    return dict(nominal=nominal, stacks=stacks, counts=counts, p_gate=counts.to(torch.float64) / int(trials), flips=flips,
                rects=rects.view(int(trials), k - 1, max_rects, 4), rect_counts=rect_counts.view(int(trials), k - 1))


def _experiment_boxes(rects, cfg, merge_flag, frame_hw):
    """The boxes of every pair from its ROI rectangles, as the scripts' ``task_results`` form them: the union box (FLAG 2,
    the one rectangle of the device table), every rectangle (FLAG 1) or their padded bounding box (FLAG 1 merged)."""
    return [prediction_boxes(rs, len(rs) + 1, 1, merge_flag, frame_hw) if cfg.FLAG == 1 else rs for rs in rects]


def prediction_sequence_dev(frames_bgr, mem_state, cfg, with_original=True, merge_flag=True, max_rects=32, ctx=None,
                            with_viz=False):
    """``run_prediction``'s experiment for a whole sequence in HBM: ``frames_bgr`` uint8 CUDA tensor [n][H][W][3] (BGR as
    ``cv2.imread`` gives them), ``mem_state`` the ``constructed3DMatrix`` stack.  Gray frames, gating table, ROI and
    full-frame flows as ``_sequence_flows`` computes them, then one prediction warp and one SSIM launch pair per path for
    all pairs (``predict.predict_sequence_dev`` reading the same table, ``predict.ssim_batch_dev`` against frames
    2 .. n-1).  Only the slices go up and the rectangle table comes back (one copy, which also gives the host lists).
    Returns a dict of CUDA tensors -- ``pred_mem`` / ``pred_orig`` uint8 [n-2][H][W][3], ``ssim_mem`` / ``ssim_orig``
    float64 [n-2], ``flow_mem`` / ``flow_orig`` float32 [n-2][H][W][2] (the un-negated Farneback flow; the ``orig``
    entries are None without ``with_original``) -- and the host lists ``rects`` (the ROI rectangles of every pair) and
    ``boxes`` (the boxes its prediction warped, ``prediction_boxes``); equal to ``run_prediction`` with the GPU backends,
    bit for bit.  ``with_viz`` adds ``viz_mem`` / ``viz_orig``, uint8 [n-2][H][W][3]: the script's ``viz`` of the
    negated flows (:524, :578) in the B,G,R order it saves (``flowviz.flow_to_image_dev``, one call per path;
    ``flowviz.save_viz`` writes them).  Synchronises at the end, so the tensors can be read at once."""
    import torch

    from . import flowviz, predict
    from .context import default_context
    ctx = ctx or default_context()
    gray, counts, rtab, rects, flow_mem, flow_orig, gf = _sequence_flows(frames_bgr, mem_state, cfg, with_original,
                                                                         max_rects, ctx, "prediction_sequence_dev")
    n, H, W = (int(v) for v in frames_bgr.shape[:3])  # noqa: N806
    dev = frames_bgr.device
    pred_mem = torch.empty((n - 2, H, W, 3), dtype=torch.uint8, device=dev)
    ssim_mem = torch.empty((n - 2,), dtype=torch.float64, device=dev)
    if with_original:
        pred_orig = torch.empty_like(pred_mem)
        ssim_orig = torch.empty_like(ssim_mem)
    else:
        pred_orig = ssim_orig = None
    if with_viz:
        viz_mem = torch.empty_like(pred_mem)
        viz_orig = torch.empty_like(pred_mem) if with_original else None
    torch.cuda.synchronize(dev)
    predict.predict_sequence_dev(frames_bgr, flow_mem, pred_mem, counts=counts, rects=rtab, gate_frame=gf,
                                 merge_padding=PREDICT_PADDING if cfg.FLAG == 1 and merge_flag else None, ctx=ctx)
    predict.ssim_batch_dev(pred_mem, frames_bgr[2:], out=ssim_mem, ctx=ctx)
    if with_original:
        predict.predict_sequence_dev(frames_bgr, flow_orig, pred_orig, border_mode=predict.BORDER_CONSTANT, ctx=ctx)
        predict.ssim_batch_dev(pred_orig, frames_bgr[2:], out=ssim_orig, ctx=ctx)
    if with_viz:
        flowviz.flow_to_image_dev(flow_mem, viz_mem, sign=-1, convert_to_bgr=True, ctx=ctx)
        if with_original:
            flowviz.flow_to_image_dev(flow_orig, viz_orig, sign=-1, convert_to_bgr=True, ctx=ctx)
    ctx.synchronize()
    res = dict(pred_mem=pred_mem, pred_orig=pred_orig, ssim_mem=ssim_mem, ssim_orig=ssim_orig, flow_mem=flow_mem,
               flow_orig=flow_orig, rects=rects, boxes=_experiment_boxes(rects, cfg, merge_flag, (H, W)))
    if with_viz:
        res.update(viz_mem=viz_mem, viz_orig=viz_orig)
    return res


def segmentation_sequence_dev(frames_bgr, gt_masks_bgr, mem_state, cfg, with_original=True, merge_flag=False, seg_th=1,
                              max_rects=32, ctx=None, timings=None):
    """``run_segmentation``'s experiment for a whole sequence in HBM: ``frames_bgr`` and ``gt_masks_bgr`` uint8 CUDA
    tensors [n][H][W][3] (as ``cv2.imread`` gives them), ``mem_state`` the ``constructed3DMatrix`` stack.  Gray frames,
    gating table, ROI and full-frame flows as ``_sequence_flows`` computes them; then per path ONE segmentation call
    over all pairs (``segment.motion_mask_sequence_dev``: the Mem path on the boxes ``task_results`` forms from each
    pair's rectangles, the Original path on the whole frame) and ONE pixel-accuracy call against ground-truth frames
    1 .. n-2 (``segment.pixel_accuracy_batch_dev``).  Returns a dict: ``mask_mem`` / ``mask_orig`` uint8 [n-2][H][W],
    ``pa_mem`` / ``pa_orig`` float64 [n-2], ``flow_mem`` / ``flow_orig`` float32 [n-2][H][W][2] (CUDA tensors; the
    ``orig`` entries are None without ``with_original``), the host lists ``rects`` and ``boxes``, and ``mean_mem`` /
    ``mean_orig``, the two means ``run_segmentation`` returns.  Equal to ``run_segmentation`` with the GPU backends, bit
    for bit.  ``timings`` (a dict) receives the wall time of the flow stage and of the mask + accuracy stage of each
    path.  Synchronises at the end."""
    import time

    import torch

    from . import predict, segment
    from .context import default_context
    ctx = ctx or default_context()
    predict._u8_frames(gt_masks_bgr, "segmentation_sequence_dev")
    if gt_masks_bgr.dim() != 4 or tuple(gt_masks_bgr.shape) != tuple(frames_bgr.shape):
        raise predict.NsofValueError(f"segmentation_sequence_dev: ground truth {tuple(gt_masks_bgr.shape)} does not match "
                                     f"the frames {tuple(frames_bgr.shape)}")
    t0 = time.perf_counter()
    gray, counts, rtab, rects, flow_mem, flow_orig, gf = _sequence_flows(frames_bgr, mem_state, cfg, with_original,
                                                                         max_rects, ctx, "segmentation_sequence_dev")
    n, H, W = (int(v) for v in frames_bgr.shape[:3])  # noqa: N806
    dev = frames_bgr.device
    boxes = _experiment_boxes(rects, cfg, merge_flag, (H, W))
    mask_mem = torch.empty((n - 2, H, W), dtype=torch.uint8, device=dev)
    pa_mem = torch.empty((n - 2,), dtype=torch.float64, device=dev)
    mask_orig = torch.empty_like(mask_mem) if with_original else None
    pa_orig = torch.empty_like(pa_mem) if with_original else None
    torch.cuda.synchronize(dev)
    t1 = time.perf_counter()
    gt = gt_masks_bgr[1:n - 1]
    segment.motion_mask_sequence_dev(flow_mem, boxes, mask_mem, seg_th, ctx=ctx)
    segment.pixel_accuracy_batch_dev(mask_mem, gt, pa_mem, ctx=ctx)
    ctx.synchronize()
    t2 = time.perf_counter()
    if with_original:
        segment.motion_mask_sequence_dev(flow_orig, None, mask_orig, seg_th, ctx=ctx)
        segment.pixel_accuracy_batch_dev(mask_orig, gt, pa_orig, ctx=ctx)
    ctx.synchronize()
    t3 = time.perf_counter()
    if timings is not None:
        timings.update(flow_s=t1 - t0, seg_mem_s=t2 - t1, seg_orig_s=t3 - t2, pairs=n - 2)

    def mean(t):   # run_segmentation's running sum, in pair order
        acc = 0.0
        for v in t.cpu().tolist():
            acc += v
        return acc / max(n - 2, 1)
    return dict(mask_mem=mask_mem, mask_orig=mask_orig, pa_mem=pa_mem, pa_orig=pa_orig, flow_mem=flow_mem,
                flow_orig=flow_orig, rects=rects, boxes=boxes, mean_mem=mean(pa_mem),
                mean_orig=mean(pa_orig) if with_original else None)
