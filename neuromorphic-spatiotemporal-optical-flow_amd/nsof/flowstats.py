"""Statistics of an ensemble of flow fields against a reference flow (``nsof_flow_ensemble_dev``, csrc/flow_ensemble.hip;
DESIGN.md section 5.7): what device spread and write noise of the synaptic array do to the flow itself.

``flow_ensemble_dev`` folds the trials' flow fields into per-pixel moments of their deviation from the reference and
per-(trial, field) end-point-error figures in one streaming pass; ``flow_ensemble_summary`` turns the moments into mean,
covariance and error maps (plain torch, not a hot path); ``events_flow_variability_dev`` runs the whole Monte-Carlo study
of an event stream -- nominal run, trial accumulator, trial flows, reduction -- without the ensemble ever existing at once.
"""
import numpy as np

from . import _lib
from .errors import NsofValueError

_STATE = (("sum", 2), ("sq", 3), ("epe2_max", None))   # the per-pixel state arrays and their innermost dimension
_FLOW_BYTES_PER_CHUNK = 1 << 30                          # events_flow_variability_dev: the trial flows of one pair held at once


def _check_flows(who, name, t, dims, like=None):
    """``t``: a float32 CUDA tensor of ``dims`` dimensions, the last two dense ([W][2]); on ``like``'s device."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NsofValueError(f"{who}: {name} must be a CUDA tensor", _lib.NSOF_EINVAL)
    if t.dtype != torch.float32:
        raise NsofValueError(f"{who}: float32 {name} expected (got {t.dtype})", _lib.NSOF_EINVAL)
    if t.dim() != dims or t.shape[-1] != 2 or min(t.shape) < 1 or t.stride(-1) != 1 or t.stride(-2) != 2:
        lead = "[T][F]" if dims == 5 else "[F]"
        raise NsofValueError(f"{who}: {name} must be {lead}[H][W][2] with dense rows (got {tuple(t.shape)}, strides "
                             f"{tuple(t.stride())})", _lib.NSOF_ESHAPE)
    if like is not None and t.device != like.device:
        raise NsofValueError(f"{who}: {name} is on {t.device}, flows on {like.device}", _lib.NSOF_EINVAL)


def _check_tau(who, tau):
    if isinstance(tau, (bool, np.bool_)) or not isinstance(tau, (int, float, np.integer, np.floating)) or not float(tau) >= 0:
        raise NsofValueError(f"{who}: tau = {tau!r} is not a number >= 0", _lib.NSOF_EINVAL)
    return float(tau)


def _fold(ctx, flows, ref, tau, accumulate, sum_, sq, epe2_max, aee, outliers, nonfinite):
    """One ``nsof_flow_ensemble_dev`` call: ``flows`` [T][F][H][W][2], ``ref`` [F][H][W][2] or None, the state tensors dense
    [F][H][W][..], the per-trial outputs dense, ``T * F`` elements each.  Everything checked by the caller."""
    from .context import dev_ptr
    n_t, n_f, h, w = (int(v) for v in flows.shape[:4])
    rc = ctx._lib.nsof_flow_ensemble_dev(
        ctx.ptr, n_t, n_f, dev_ptr(flows), int(flows.stride(2)), int(flows.stride(1)), int(flows.stride(0)), w, h,
        dev_ptr(ref), 0 if ref is None else int(ref.stride(1)), 0 if ref is None else int(ref.stride(0)), float(tau),
        int(accumulate), dev_ptr(sum_), dev_ptr(sq), dev_ptr(epe2_max), dev_ptr(aee), dev_ptr(outliers), dev_ptr(nonfinite))
    ctx.check(rc, "flow_ensemble_dev")


def flow_ensemble_dev(flows, ref=None, tau=1.0, state=None, *, ctx=None):
    """Fold the flow fields of ``T`` trials into statistics of their deviation from ``ref`` (``nsof_flow_ensemble_dev``).
    ``flows``: float32 CUDA tensor ``[T][F][H][W][2]``, (u, v) interleaved; trial, field and row strides may be padded, the
    innermost two dimensions are dense.  ``ref``: ``[F][H][W][2]`` likewise, or ``None`` for a zero reference.  With
    ``du = flow.u - ref.u``, ``dv`` likewise and ``e2 = du*du + dv*dv``, all in float64, returns a dict of CUDA tensors:
    ``sum`` float64 ``[F][H][W][2]`` (sum of du, dv over the trials), ``sq`` ``[F][H][W][3]`` (du*du, dv*dv, du*dv),
    ``epe2_max`` ``[F][H][W]`` (largest e2; a NaN never enters it, +inf does), and per trial and field ``aee`` float64
    ``[T][F]`` (mean of sqrt(e2) over the pixels), ``outliers`` int32 (pixels with ``e2 > tau*tau``) and ``nonfinite`` int32
    (pixels whose e2 is NaN or infinite: such a trial's ``aee`` is not finite); ``n_trials``: the count folded so far.
    ``state=`` a previous result continues it: its ``sum``, ``sq`` and ``epe2_max`` are updated in place (and returned),
    ``n_trials`` is added up, the per-trial outputs are those of this call's trials.  The trials are folded in index order
    and the pixel sum of ``aee`` has a fixed order, so a run cut into calls at any trials equals the one-shot call bit for
    bit, and two runs give the same bits.  Shapes, dtypes or devices that do not match raise ``NsofValueError`` before the
    library is called.  Asynchronous on the context's stream: ``ctx.synchronize()`` before reading the results elsewhere."""
    import torch

    from .context import default_context
    who = "flow_ensemble_dev"
    _check_flows(who, "flows", flows, 5)
    if ref is not None:
        _check_flows(who, "ref", ref, 4, like=flows)
        if tuple(ref.shape) != tuple(flows.shape[1:]):
            raise NsofValueError(f"{who}: ref is {tuple(ref.shape)}, the flows' fields are {tuple(flows.shape[1:])}", _lib.NSOF_ESHAPE)
    tau = _check_tau(who, tau)
    n_t, n_f, h, w = (int(v) for v in flows.shape[:4])
    shapes = {k: (n_f, h, w) + ((c,) if c else ()) for k, c in _STATE}
    if state is not None:
        try:
            arrays, done = [state[k] for k, _ in _STATE], state["n_trials"]
        except (KeyError, TypeError, IndexError):
            raise NsofValueError(f"{who}: state must be a result of {who} (sum, sq, epe2_max, n_trials)", _lib.NSOF_EINVAL) from None
        for (k, _), a in zip(_STATE, arrays):
            if not isinstance(a, torch.Tensor) or a.dtype != torch.float64 or a.device != flows.device or \
                    tuple(a.shape) != shapes[k] or not a.is_contiguous():
                raise NsofValueError(f"{who}: state[{k!r}] must be a contiguous float64 tensor {shapes[k]} on {flows.device}",
                                     _lib.NSOF_ESHAPE)
        if isinstance(done, (bool, np.bool_)) or not isinstance(done, (int, np.integer)) or done < 0:
            raise NsofValueError(f"{who}: state['n_trials'] = {done!r} is not a whole number >= 0", _lib.NSOF_EINVAL)
    else:
        arrays, done = [torch.empty(shapes[k], dtype=torch.float64, device=flows.device) for k, _ in _STATE], 0
    aee = torch.empty((n_t, n_f), dtype=torch.float64, device=flows.device)
    outliers, nonfinite = (torch.empty((n_t, n_f), dtype=torch.int32, device=flows.device) for _ in range(2))
    torch.cuda.synchronize(flows.device)   # the library writes on the context's stream
    _fold(ctx or default_context(), flows, ref, tau, state is not None, *arrays, aee, outliers, nonfinite)
    return dict(sum=arrays[0], sq=arrays[1], epe2_max=arrays[2], aee=aee, outliers=outliers, nonfinite=nonfinite,
                n_trials=int(done) + n_t)


def flow_ensemble_summary(res, ref=None):
    """The moments of ``flow_ensemble_dev`` as maps (float64 torch expressions on the tensors' device; the caller has
    synchronised the context): ``mean`` ``[..][H][W][2]`` = ``ref + sum / n`` (``ref=None``: zero), ``cov`` ``[..][H][W][2][2]`` the
    sample covariance of (u, v) per pixel, ``(sq - sum sum^T / n) / (n - 1)`` (needs ``n >= 2``), ``epe_rms`` =
    ``sqrt((sq.uu + sq.vv) / n)`` and ``epe_max`` = ``sqrt(epe2_max)``, the root-mean-square and the largest end-point
    error against the reference."""
    import torch
    n = res["n_trials"]
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 2:
        raise NsofValueError(f"flow_ensemble_summary: n_trials = {n!r}, the sample covariance needs at least 2", _lib.NSOF_EINVAL)
    s, q = res["sum"], res["sq"]
    if ref is not None and tuple(ref.shape) != tuple(s.shape):
        raise NsofValueError(f"flow_ensemble_summary: ref is {tuple(ref.shape)}, the statistics' fields are {tuple(s.shape)}",
                             _lib.NSOF_ESHAPE)
    d = s / n
    mean = d if ref is None else ref.to(torch.float64) + d
    cuu = (q[..., 0] - s[..., 0] * d[..., 0]) / (n - 1)
    cvv = (q[..., 1] - s[..., 1] * d[..., 1]) / (n - 1)
    cuv = (q[..., 2] - s[..., 0] * d[..., 1]) / (n - 1)
    cov = torch.stack((torch.stack((cuu, cuv), -1), torch.stack((cuv, cvv), -1)), -2)
    return dict(mean=mean, cov=cov, epe_rms=torch.sqrt((q[..., 0] + q[..., 1]) / n), epe_max=torch.sqrt(res["epe2_max"]))


def _trial_chunk_arg(trial_chunk, trials, h, w):
    """Trials whose flows of one pair are formed at a time: all of them if they fit in 1 GiB, else the most that do."""
    if trial_chunk is None:
        return max(1, min(trials, _FLOW_BYTES_PER_CHUNK // (8 * h * w)))
    if isinstance(trial_chunk, (bool, np.bool_)) or not isinstance(trial_chunk, (int, np.integer)) or trial_chunk < 1:
        raise NsofValueError(f"events_flow_variability_dev: trial_chunk = {trial_chunk!r} is not a whole number >= 1", _lib.NSOF_EINVAL)
    return min(int(trial_chunk), trials)


def events_flow_variability_dev(x, y, p, t, sensor_hw, rel_sigma, trials, seed=0, params=None, slice_us=1000, active_v=-6.0,
                                silent_v=0.0, snapshot_every=33, accum_params=None, dt=None, refractory_us=None,
                                theta_events=None, c2c=None, tau=1.0, trial_chunk=None, ctx=None, timings=None):
    """What device-to-device variability and write noise do to the FLOW of an event stream, in HBM -- the event pipeline of
    ``events_to_flow_sequence`` (BASELINE config 5) as a Monte-Carlo study.  The nominal array (``accum_params``; ``None``:
    ``PARAMS``) gives ``frames_nominal`` uint8 ``[n][H][W]`` and ``flow_nominal`` float32 ``[n-1][H][W][2]`` exactly as
    ``events_to_flow_sequence`` with the same arguments (``params``: the Farneback parameters).  The ``trials`` arrays --
    ``TrialAccumulator(H, W, maps, version=1, trials=trials, c2c=c2c, ...)`` with ``maps`` =
    ``variability_maps(H, W, rel_sigma, accum_params, seed, trials=trials)`` less the keys whose spread is 0 -- are stepped one
    snapshot interval at a time and their 8-bit surfaces taken after each (``surface_u8_dev``) into two alternating stacks;
    the ``T`` flows of pair ``(k, k+1)`` (``farneback_batch`` over the two stacks: trial ``t``'s flow has the bits
    ``farneback_sequence`` over trial ``t``'s surfaces gives) are formed ``trial_chunk`` trials at a time (``None``: all, if
    their flows of one pair fit in 1 GiB, else the most that do) and folded into that pair's statistics with ``ref =
    flow_nominal[k]`` (``flow_ensemble_dev``), the state continued from chunk to chunk.  Besides the nominal run and the
    statistics, no more than ``trial_chunk`` flow fields and two surfaces per trial exist at any point.
    Returns a dict of CUDA tensors: ``frames_nominal``, ``flow_nominal``, ``sum`` float64 ``[n-1][H][W][2]``, ``sq``
    ``[n-1][H][W][3]``, ``epe2_max`` ``[n-1][H][W]``, ``aee`` float64 ``[T][n-1]``, ``outliers`` and ``nonfinite`` int32 ``[T][n-1]``
    (``tau``: the outlier threshold in pixels), and ``n_trials``; ``flow_ensemble_summary(res, res["flow_nominal"])`` gives the
    maps.  The result does not depend on ``trial_chunk``, bit for bit.  An empty or all-zero ``rel_sigma`` with ``c2c=None``
    still takes the trial run: identical devices, every statistic exactly 0.  ``timings`` (a dict) receives the wall time of
    the stages.  Every refusal of the arguments comes before any device work.  Synchronises at the end."""
    import time

    import torch

    from .accumulator import TrialAccumulator, c2c_arg, slice_index_array, variability_maps
    from .context import default_context
    from .farneback import PARAMS_A, farneback_batch
    from .pipeline import events_to_flow_sequence
    who = "events_flow_variability_dev"
    H, W = (int(v) for v in sensor_hw)  # noqa: N806
    variability_maps(1, 1, rel_sigma, accum_params, seed, trials=trials)   # refuses before any device work
    c2c_arg(c2c)                                                            # ... and so does this
    for name, v in (("active_v", active_v), ("silent_v", silent_v)):
        if isinstance(v, (str, bytes)) or np.ndim(v) != 0:
            raise NsofValueError(f"{who}: {name} = {v!r} must be one number -- the nominal array has one operating "
                                 "point; a voltage per trial is TrialAccumulator's / simulate_trials_dev's")
    tau = _check_tau(who, tau)
    trials = int(trials)
    chunk = _trial_chunk_arg(trial_chunk, trials, H, W)
    ctx = ctx or default_context()
    params = params or PARAMS_A
    dev = torch.device("cuda", ctx.device)
    t0 = time.perf_counter()
    frames, flow_nominal = events_to_flow_sequence(x, y, p, t, (H, W), params, slice_us, active_v, silent_v, snapshot_every,
                                                   ctx=ctx, accum_params=accum_params, dt=dt, refractory_us=refractory_us,
                                                   theta_events=theta_events)
    t1 = time.perf_counter()
    n = int(frames.shape[0])
    idx = slice_index_array(t, slice_us, ctx)
    # the planes of the keys that do vary (events_variability_dev: a key's plane does not depend on which other spreads are zero)
    maps = {k: v for k, v in variability_maps(H, W, rel_sigma, accum_params, seed, trials=trials).items() if float(rel_sigma[k]) != 0.0}
    stats = {k: torch.empty((n - 1, H, W) + ((c,) if c else ()), dtype=torch.float64, device=dev) for k, c in _STATE}
    # per pair, then per trial: a chunk's figures of one pair are consecutive, as the library writes them
    aee = torch.empty((n - 1, trials), dtype=torch.float64, device=dev)
    outliers, nonfinite = (torch.empty((n - 1, trials), dtype=torch.int32, device=dev) for _ in range(2))
    surfaces = [torch.empty((trials, H, W), dtype=torch.uint8, device=dev) for _ in range(2)]
    flows = torch.empty((chunk, 1, H, W, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)   # the library writes on the context's stream
    t_acc = t_flow = t_fold = 0.0
    acc = TrialAccumulator(H, W, maps, version=1, active_v=active_v, silent_v=silent_v, trials=trials, c2c=c2c,
                           params=accum_params, dt=dt, refractory_us=refractory_us, theta_events=theta_events, ctx=ctx)
    try:
        for k in range(n):
            ta = time.perf_counter()
            acc.step(x, y, p, t, idx[k * snapshot_every:(k + 1) * snapshot_every + 1])
            prev, cur = surfaces[(k - 1) & 1], acc.surface_u8_dev(out=surfaces[k & 1])
            if timings is not None:
                ctx.synchronize()
            t_acc += time.perf_counter() - ta
            for c0 in range(0, trials if k else 0, chunk):
                c1 = min(c0 + chunk, trials)
                tb = time.perf_counter()
                farneback_batch(prev[c0:c1], cur[c0:c1], flows, c1 - c0, H, W, params, ctx=ctx)
                if timings is not None:
                    ctx.synchronize()
                tc = time.perf_counter()
                _fold(ctx, flows[:c1 - c0], flow_nominal[k - 1:k], tau, c0 > 0, *(stats[s][k - 1:k] for s, _ in _STATE),
                      aee[k - 1, c0:c1], outliers[k - 1, c0:c1], nonfinite[k - 1, c0:c1])
                if timings is not None:
                    ctx.synchronize()
                t_flow += tc - tb
                t_fold += time.perf_counter() - tc
        ctx.synchronize()
    finally:
        acc.close()
    if timings is not None:
        timings.update(nominal_s=t1 - t0, trial_accumulator_s=t_acc, trial_flows_s=t_flow, ensemble_s=t_fold, frames=n,
                       trials=trials, trial_chunk=chunk)
    return dict(frames_nominal=frames, flow_nominal=flow_nominal, **stats, aee=aee.t().contiguous(),
                outliers=outliers.t().contiguous(), nonfinite=nonfinite.t().contiguous(), n_trials=trials)
