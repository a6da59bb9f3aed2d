"""GPU: nsof_flow_ensemble_dev / nsof.flow_ensemble_dev against the NumPy restatement (tests/flow_ensemble_ref.py) bit for
bit -- aee within the bound of any summation order --, its chunking, non-finite and refusal contracts, and
nsof.events_flow_variability_dev against the study done the long way (TrialAccumulator stepped by hand, farneback_sequence
per trial, the restatement)."""
import ctypes as C

import numpy as np
import pytest

import flow_ensemble_ref as R

pytestmark = pytest.mark.gpu

CASES = R.kernel_cases()
STATE = ("sum", "sq", "epe2_max")
PER_TRIAL = ("aee", "outliers", "nonfinite")
TAU = 14.0   # with flows and reference in +-20 px the end-point error spreads over 0..56: outliers are neither none nor all


@pytest.fixture(scope="module")
def ensembles():
    """case -> (flows, ref, restatement with the reference, restatement without); computed once, never changed."""
    out = {}
    for i, case in enumerate(CASES):
        flows, ref = R.make_flows(case, 100 + i)
        out[case] = (flows, ref, R.fold(flows, ref, TAU), R.fold(flows, None, TAU))
    return out


def _strided(torch, dev, a, strides, fill=float("nan")):
    """``a`` on the device as a view with the given element strides of its leading dimensions (the last two dense) into a
    buffer whose padding holds ``fill``; the buffer ends with the view's last element."""
    lead = a.shape[:-2]
    size = sum((n - 1) * s for n, s in zip(lead, strides)) + a.shape[-2] * 2
    buf = torch.full((size,), fill, dtype=torch.float32, device=dev)
    view = buf.as_strided(a.shape, tuple(strides) + (2, 1))
    view.copy_(torch.from_numpy(a))
    return view


def _upload(torch, dev, case, flows, ref, padded):
    t, f, h, w = case
    rs, fs, ts = R.strides(case, padded)
    d_flows = _strided(torch, dev, flows, (ts, fs, rs))
    d_ref = None if ref is None else _strided(torch, dev, ref, (h * (2 * w + 2) + 2, 2 * w + 2) if padded else (h * 2 * w, 2 * w))
    return d_flows, d_ref


def _host(ctx, res):
    ctx.synchronize()
    return {k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in res.items()}


def _assert_equals_restatement(got, want, case, equal_nan=False):
    t, f, h, w = case
    for k in STATE + ("outliers", "nonfinite"):
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k], equal_nan=equal_nan), k
    assert got["n_trials"] == want["n_trials"]
    fin = np.isfinite(want["aee"])
    assert np.array_equal(np.isfinite(got["aee"]), fin)
    err = np.abs(got["aee"][fin] - want["aee"][fin])
    print(f"case {case}: aee max rel err {np.max(err / want['aee'][fin], initial=0.0):.3g}, bound {R.aee_bound(w, h):.3g}")
    assert (err <= R.aee_bound(w, h) * want["aee"][fin]).all()


@pytest.mark.parametrize("with_ref", [True, False], ids=["ref", "noref"])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_matches_restatement(nsof_lib, ctx, torch_dev, ensembles, case, padded, with_ref):
    import torch
    flows, ref, want_ref, want_zero = ensembles[case]
    d_flows, d_ref = _upload(torch, torch_dev, case, flows, ref if with_ref else None, padded)
    got = _host(ctx, nsof_lib.flow_ensemble_dev(d_flows, d_ref, TAU, ctx=ctx))
    _assert_equals_restatement(got, want_ref if with_ref else want_zero, case)
    assert 0 < got["outliers"].sum() < got["outliers"].size * case[2] * case[3] or case[2] * case[3] == 1
    again = _host(ctx, nsof_lib.flow_ensemble_dev(d_flows, d_ref, TAU, ctx=ctx))
    for k in STATE + PER_TRIAL:
        assert np.array_equal(again[k], got[k]), f"{k} differs between two calls"


@pytest.mark.parametrize("cuts", [(2,), (1, 2, 3, 4)], ids=["2+3", "1+1+1+1+1"])
@pytest.mark.parametrize("padded", [False, True], ids=["dense", "padded"])
def test_chunked_equals_one_shot(nsof_lib, ctx, torch_dev, ensembles, padded, cuts):
    import torch
    case = (5, 2, 19, 37)
    flows, ref, want, _ = ensembles[case]
    d_flows, d_ref = _upload(torch, torch_dev, case, flows, ref, padded)
    whole = _host(ctx, nsof_lib.flow_ensemble_dev(d_flows, d_ref, TAU, ctx=ctx))
    state, parts = None, []
    for a, b in zip((0,) + cuts, cuts + (5,)):
        state = nsof_lib.flow_ensemble_dev(d_flows[a:b], d_ref, TAU, state=state, ctx=ctx)
        parts.append(_host(ctx, {k: state[k] for k in PER_TRIAL}))
    got = _host(ctx, state)
    assert got["n_trials"] == 5
    for k in STATE:
        assert np.array_equal(got[k], whole[k]), k
    for k in PER_TRIAL:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    _assert_equals_restatement(dict(got, **{k: whole[k] for k in PER_TRIAL}), want, case)


def test_state_must_match(nsof_lib, ctx, torch_dev, ensembles):
    import torch
    case = (5, 2, 19, 37)
    flows, ref, _, _ = ensembles[case]
    d_flows, d_ref = _upload(torch, torch_dev, case, flows, ref, False)
    state = nsof_lib.flow_ensemble_dev(d_flows, d_ref, TAU, ctx=ctx)
    err = nsof_lib.errors.NsofValueError
    with pytest.raises(err, match="state"):
        nsof_lib.flow_ensemble_dev(d_flows[:, :1], d_ref[:1], TAU, state=state, ctx=ctx)
    with pytest.raises(err, match="state"):
        nsof_lib.flow_ensemble_dev(d_flows, d_ref, TAU, state=dict(state, sq=state["sq"].to(torch.float32)), ctx=ctx)
    with pytest.raises(err, match="state"):
        nsof_lib.flow_ensemble_dev(d_flows, d_ref, TAU, state=dict(sum=state["sum"]), ctx=ctx)
    with pytest.raises(err, match="ref"):
        nsof_lib.flow_ensemble_dev(d_flows, d_ref[:1], TAU, ctx=ctx)
    with pytest.raises(err, match="float32"):
        nsof_lib.flow_ensemble_dev(d_flows.to(torch.float64), d_ref, TAU, ctx=ctx)
    with pytest.raises(err, match="dense rows"):
        nsof_lib.flow_ensemble_dev(d_flows[:, :, :, ::2], None, TAU, ctx=ctx)
    with pytest.raises(err, match="tau"):
        nsof_lib.flow_ensemble_dev(d_flows, d_ref, -1.0, ctx=ctx)


def test_non_finite_input(nsof_lib, ctx, torch_dev, ensembles):
    """Trial 2, field 0: a NaN u at one pixel and a +inf u at another.  IEEE decides those two pixels' sum and sq; the
    maximum skips the NaN and takes the inf; nothing else moves."""
    import torch
    case = (5, 2, 19, 37)
    clean_flows, ref, clean, _ = ensembles[case]
    flows = clean_flows.copy()
    nan_px, inf_px = (0, 3, 4), (0, 7, 20)
    flows[(2,) + nan_px + (0,)] = np.nan
    flows[(2,) + inf_px + (0,)] = np.inf
    d_flows, d_ref = _upload(torch, torch_dev, case, flows, ref, False)
    got = _host(ctx, nsof_lib.flow_ensemble_dev(d_flows, d_ref, TAU, ctx=ctx))
    _assert_equals_restatement(got, R.fold(flows, ref, TAU), case, equal_nan=True)
    # ... and spelled out
    assert np.isnan(got["sum"][nan_px][0]) and np.isnan(got["sq"][nan_px][[0, 2]]).all()
    assert np.array_equal(got["sum"][nan_px][1], clean["sum"][nan_px][1]) and got["sq"][nan_px][1] == clean["sq"][nan_px][1]
    assert got["sum"][inf_px][0] == np.inf and got["sq"][inf_px][0] == np.inf and np.isinf(got["sq"][inf_px][2])
    others = R.fold(np.delete(flows, 2, axis=0), ref, TAU)["epe2_max"]
    assert got["epe2_max"][nan_px] == others[nan_px] and got["epe2_max"][inf_px] == np.inf
    mask = np.ones(clean["epe2_max"].shape, bool)
    mask[nan_px] = mask[inf_px] = False
    for k in STATE:
        assert np.array_equal(got[k][mask], clean[k][mask]), k
    want_nonfinite = np.zeros((5, 2), np.int32)
    want_nonfinite[2, 0] = 2
    assert np.array_equal(got["nonfinite"], want_nonfinite)
    assert np.array_equal(np.isfinite(got["aee"]), want_nonfinite == 0)
    keep = want_nonfinite == 0
    assert np.array_equal(got["aee"][keep], _host(ctx, nsof_lib.flow_ensemble_dev(
        _upload(torch, torch_dev, case, clean_flows, ref, False)[0], d_ref, TAU, ctx=ctx))["aee"][keep])


def _refusal_cases():
    nan = float("nan")
    for k, v in (("n_trials", 0), ("n_fields", 0), ("width", 0), ("height", 0), ("n_trials", -1), ("n_fields", -3),
                 ("width", -1), ("height", -2)):
        yield f"{k}={v}", {k: v}, "EINVAL", str(v)
    for k in ("flows", "sum", "sq", "epe2_max", "aee", "outliers", "nonfinite"):
        yield f"null {k}", {k: None}, "EINVAL", k
    yield "odd row stride", dict(rs=2 * 9 + 1), "EINVAL", "19"
    yield "short row stride", dict(rs=2 * 9 - 2), "EINVAL", "16"
    yield "odd reference row stride", dict(rrs=2 * 9 + 1), "EINVAL", "19"
    yield "accumulate 2", dict(accumulate=2), "EINVAL", "2"
    yield "accumulate -1", dict(accumulate=-1), "EINVAL", "-1"
    yield "tau negative", dict(tau=-0.5), "EINVAL", "-0.5"
    yield "tau NaN", dict(tau=nan), "EINVAL", "nan"
    yield "W*H > 2^27", dict(width=1 << 14, height=(1 << 13) + 1, rs=2 << 14, rrs=2 << 14), "EUNSUPPORTED", "2^27"
    yield "height beyond one launch", dict(width=1, height=300_000), "EUNSUPPORTED", "300000"


@pytest.mark.parametrize("name, change, status, named", list(_refusal_cases()), ids=[c[0] for c in _refusal_cases()])
def test_refusals_leave_the_outputs_untouched(nsof_lib, ctx, torch_dev, name, change, status, named):
    """Every refusal of include/nsof.h, one at a time: the status, the offending value in nsof_last_error, and all six
    outputs -- pre-filled with 7 -- still 7.  (Nothing is launched, so the sizes the refused calls name are never touched.)"""
    import torch
    from nsof import _lib
    t, f, h, w = 3, 2, 5, 9
    flows = torch.zeros((t, f, h, w, 2), dtype=torch.float32, device=torch_dev)
    ref = torch.zeros((f, h, w, 2), dtype=torch.float32, device=torch_dev)
    outs = dict(sum=torch.full((f, h, w, 2), 7.0, dtype=torch.float64, device=torch_dev),
                sq=torch.full((f, h, w, 3), 7.0, dtype=torch.float64, device=torch_dev),
                epe2_max=torch.full((f, h, w), 7.0, dtype=torch.float64, device=torch_dev),
                aee=torch.full((t, f), 7.0, dtype=torch.float64, device=torch_dev),
                outliers=torch.full((t, f), 7, dtype=torch.int32, device=torch_dev),
                nonfinite=torch.full((t, f), 7, dtype=torch.int32, device=torch_dev))
    torch.cuda.synchronize(torch_dev)
    a = dict(n_trials=t, n_fields=f, flows=flows.data_ptr(), rs=2 * w, fs=h * 2 * w, ts=f * h * 2 * w, width=w, height=h,
             ref=ref.data_ptr(), rrs=2 * w, rfs=h * 2 * w, tau=1.0, accumulate=0, **{k: v.data_ptr() for k, v in outs.items()})

    def call(a):
        return ctx._lib.nsof_flow_ensemble_dev(ctx.ptr, a["n_trials"], a["n_fields"], a["flows"], a["rs"], a["fs"], a["ts"],
                                               a["width"], a["height"], a["ref"], a["rrs"], a["rfs"], a["tau"], a["accumulate"],
                                               a["sum"], a["sq"], a["epe2_max"], a["aee"], a["outliers"], a["nonfinite"])
    rc = call(dict(a, **change))
    assert rc == getattr(_lib, "NSOF_" + status), name
    msg = ctx._lib.nsof_last_error(ctx.ptr).decode()
    assert "flow_ensemble" in msg and named in msg, msg
    ctx.synchronize()
    for k, v in outs.items():
        assert bool((v == 7).all()), f"{k} was written by a refused call ({name})"
    if name == "n_trials=0":   # the same arguments unchanged are accepted, with and without the reference
        assert call(a) == _lib.NSOF_OK and call(dict(a, ref=None, accumulate=1)) == _lib.NSOF_OK
        ctx.synchronize()
        assert not bool(outs["sum"].any()) and not bool(outs["aee"].any()) and not bool(outs["outliers"].any())


# ---- the pipeline ------------------------------------------------------------------------------------------------------
HW = (72, 136)
EVERY = 33


@pytest.fixture(scope="module")
def stream():
    from nsof import synth
    x, y, p, t = synth.make_events(7, width=136, height=72, n_background=2000, duration_us=200_000, box=(12, 10), speed_pps=250.0)
    assert x.size == 10_000
    return x, y, p, t


def _long_way(nsof, ctx, dev, stream, rel_sigma, trials, c2c, tau):
    """The study by hand: nominal run, the trial accumulator stepped interval by interval, farneback_sequence over each
    trial's surfaces, the restatement -> (nominal frames, trial frames [T][n][H][W], restatement with [n-1] leading)."""
    import torch
    from nsof.accumulator import slice_index_array
    from nsof.farneback import PARAMS_A
    from nsof.pipeline import events_to_flow_sequence
    x, y, p, t = stream
    h, w = HW
    frames_nom, flow_nom = events_to_flow_sequence(x, y, p, t, HW, slice_us=1000, active_v=-6.0, silent_v=0.0,
                                                   snapshot_every=EVERY, ctx=ctx)
    n = int(frames_nom.shape[0])
    assert n == 6
    maps = {k: v for k, v in nsof.variability_maps(h, w, rel_sigma, None, 0, trials=trials).items() if float(rel_sigma[k]) != 0.0}
    idx = slice_index_array(t, 1000)
    frames = torch.empty((trials, n, h, w), dtype=torch.uint8, device=dev)
    flows = torch.empty((trials, n - 1, h, w, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    acc = nsof.TrialAccumulator(h, w, maps, version=1, active_v=-6.0, silent_v=0.0, trials=trials, c2c=c2c, ctx=ctx)
    try:
        for k in range(n):
            acc.step(x, y, p, t, idx[k * EVERY:(k + 1) * EVERY + 1])
            acc.surface_u8_dev(out=frames[:, k])
        for i in range(trials):
            nsof.farneback_sequence(frames[i], flows[i], n, h, w, PARAMS_A, ctx=ctx)
        ctx.synchronize()
    finally:
        acc.close()
    want = R.fold(flows.cpu().numpy(), flow_nom.cpu().numpy(), tau)
    return frames_nom.cpu().numpy(), flow_nom.cpu().numpy(), frames.cpu().numpy(), want


def _study(nsof, ctx, stream, rel_sigma, trials, **kw):
    x, y, p, t = stream
    res = nsof.events_flow_variability_dev(x, y, p, t, HW, rel_sigma, trials, snapshot_every=EVERY, ctx=ctx, **kw)
    return {k: v.cpu().numpy() if hasattr(v, "cpu") else v for k, v in res.items()}


def _assert_study(got, frames_nom, flow_nom, want):
    h, w = HW
    assert np.array_equal(got["frames_nominal"], frames_nom) and np.array_equal(got["flow_nominal"], flow_nom)
    for k in STATE + ("outliers", "nonfinite"):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), k
    assert got["n_trials"] == want["n_trials"] and got["aee"].shape == want["aee"].shape
    err = np.abs(got["aee"] - want["aee"])
    print(f"study: aee max rel err {np.max(err / np.maximum(want['aee'], 1e-300)):.3g}, bound {R.aee_bound(w, h):.3g}")
    assert (err <= R.aee_bound(w, h) * want["aee"]).all()


TAU_STUDY = 0.5


@pytest.fixture(scope="module")
def spread_study(nsof_lib, ctx, torch_dev, stream):
    """(a): koff spread 10 %, three trials -- the long way and the entry, once."""
    long = _long_way(nsof_lib, ctx, torch_dev, stream, dict(koff=0.1), 3, None, TAU_STUDY)
    return long, _study(nsof_lib, ctx, stream, dict(koff=0.1), 3, tau=TAU_STUDY)


def test_study_equals_the_long_way(spread_study):
    (frames_nom, flow_nom, frames, want), got = spread_study
    assert any(not np.array_equal(frames[i], frames_nom) for i in range(3)), "no trial's frames differ from the nominal's"
    assert want["epe2_max"].any() and want["sum"].shape == (5, 72, 136, 2) and want["aee"].shape == (3, 5)
    _assert_study(got, frames_nom, flow_nom, want)


def test_study_does_not_depend_on_trial_chunk(nsof_lib, ctx, stream, spread_study):
    _, whole = spread_study
    for chunk in (1, 2):
        got = _study(nsof_lib, ctx, stream, dict(koff=0.1), 3, tau=TAU_STUDY, trial_chunk=chunk)
        for k in whole:
            assert np.array_equal(got[k], whole[k]), (k, chunk)


def test_study_of_identical_devices_is_zero(nsof_lib, ctx, stream):
    got = _study(nsof_lib, ctx, stream, {}, 3, tau=TAU_STUDY)
    for k in STATE + PER_TRIAL:
        assert not got[k].any(), k
    assert got["n_trials"] == 3 and got["aee"].shape == (3, 5) and got["sq"].shape == (5, 72, 136, 3)
    zero_sigma = _study(nsof_lib, ctx, stream, dict(koff=0.0, wini=0.0), 2, tau=TAU_STUDY)
    assert all(not zero_sigma[k].any() for k in STATE + PER_TRIAL)


def test_study_of_write_noise_equals_the_long_way(nsof_lib, ctx, torch_dev, stream):
    c2c = dict(sigma=0.05, seed=1)
    frames_nom, flow_nom, frames, want = _long_way(nsof_lib, ctx, torch_dev, stream, {}, 3, c2c, TAU_STUDY)
    assert want["epe2_max"].any(), "the noise does not move the flow on the long way"
    got = _study(nsof_lib, ctx, stream, {}, 3, c2c=c2c, tau=TAU_STUDY)
    _assert_study(got, frames_nom, flow_nom, want)
    assert got["epe2_max"].any()
