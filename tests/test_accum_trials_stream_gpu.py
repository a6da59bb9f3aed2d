"""GPU: the resumable trial accumulator (``nsof_accum_trials``; ``nsof.TrialAccumulator``) -- a run cut into chunks against
the run in one chunk, the checkpoint through the host, per-trial drive voltages against the NumPy restatement at each
trial's own operating point, and the trials' surfaces against ``Accumulator.surface_u8`` / ``surface_f32`` trial by trial.

Shapes: the six small cases of tests/accum_maps_cases.py (7x37, 40 slices, 1500 events) with the cuts of
tests/accum_trials_stream_cases.py, whose claims the CPU file asserts.  Device against device is bit for bit.  Device
against the restatement follows tests/test_accum_c2c_gpu.py: states bit for bit -- unless the restatement's closest midpoint
approach says a power sat on a rounding boundary (the CPU file asserts that none does for these inputs) -- and resistances
within 1 ulp."""
import ctypes as C
import functools

import numpy as np
import pytest

import accum_c2c_ref as N  # noqa: N812
import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_trials_cases as T  # noqa: N812
import accum_trials_stream_cases as S  # noqa: N812
from conftest import ulp_diff

pytestmark = pytest.mark.gpu

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same(a, b):
    """Two result dicts, bit for bit (float32 states and resistances, float64 block currents)."""
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and
                                        np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def stream(case, tail=0):
    """The case's events and slice bounds, with ``tail`` slices without events appended."""
    from nsof.accumulator import slice_index_array
    ev, _ = K.stream_of(case)
    idx = slice_index_array(ev[3], 1000)
    assert len(idx) - 1 == S.N_SLICES
    return ev, np.concatenate([idx, np.full(tail, idx[-1], np.int64)])


def make(nsof, ctx, case, trials, noise=None, active_v=K.ACTIVE_V, silent_v=None, memsize=T.MEMSIZE):
    c = K.CASES[case]
    maps = T.trial_maps(case, S.SEEDS[:trials])[0]
    return nsof.TrialAccumulator(*K.SMALL, maps, c["version"], c["polarity"], active_v, c["silent_v"] if silent_v is None else silent_v,
                                 c2c=noise, params=K.PARAMS, dt=K.DT, refractory_us=c["refractory_us"], theta_events=c["theta"],
                                 snapshot_every=T.SNAP_EVERY, memsize=memsize, ctx=ctx)


def read(acc, currents):
    import torch
    out = dict(w=acc.w_dev(), resistance=acc.resistance_dev(), block_current=torch.cat(currents, 2))
    acc.ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_chunks(nsof, ctx, case, trials, cuts=(), noise=None, tail=0, **kw):
    """The stream in chunks that end after the slices ``cuts`` -> w, resistance, the chunks' block currents concatenated."""
    ev, idx = stream(case, tail)
    acc = make(nsof, ctx, case, trials, noise, **kw)
    try:
        edges = [0, *cuts, len(idx) - 1]
        cur = [acc.step(*ev, idx[a:b + 1]) for a, b in zip(edges, edges[1:])]
        assert acc.slice_counter == len(idx) - 1
        assert [c.shape[2] for c in cur] == [S.snaps_between(a, b - a, T.SNAP_EVERY) for a, b in zip(edges, edges[1:])]
        return read(acc, cur)
    finally:
        acc.close()


@functools.lru_cache(maxsize=None)
def _one_shot(nsof, ctx, case, trials, noise_items, tail):
    return run_chunks(nsof, ctx, case, trials, (), dict(noise_items) if noise_items else None, tail)


def one_shot(nsof, ctx, case, trials, noise=None, tail=0):
    """The run in ONE step: computed once per (case, T, noise), shared, never modified."""
    return _one_shot(nsof, ctx, case, trials, S.items(noise) if noise else None, tail)


@pytest.mark.parametrize("noise", [None, N.NOISE], ids=["quiet", "noise"])
@pytest.mark.parametrize("trials", S.TRIALS)
@pytest.mark.parametrize("case", S.CASES)
def test_chunked_equals_one_shot(nsof_lib, ctx, case, trials, noise):
    want = one_shot(nsof_lib, ctx, case, trials, noise)
    assert want["w"].shape == ((2 if case == "small_v2_split" else 1), trials) + K.SMALL
    assert want["block_current"].shape == want["w"].shape[:2] + (6, K.SMALL[0] // T.MEMSIZE, K.SMALL[1] // T.MEMSIZE)
    for k in S.cuts_of(case):
        assert same(run_chunks(nsof_lib, ctx, case, trials, (k,), noise), want), k
    assert same(run_chunks(nsof_lib, ctx, case, trials, S.THREE_CHUNKS, noise), want)
    # a chunk whose slices hold no events (a leaking array still moves in them)
    longer = one_shot(nsof_lib, ctx, case, trials, noise, S.EMPTY_TAIL)
    assert same(run_chunks(nsof_lib, ctx, case, trials, (S.N_SLICES,), noise, S.EMPTY_TAIL), longer)
    assert np.array_equal(bits(longer["w"]), bits(want["w"])) == (K.CASES[case]["silent_v"] == 0.0)


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split", "small_v1_leak"])
def test_the_function_and_the_one_shot_entry_give_the_object_s_bits(nsof_lib, ctx, case):
    """``simulate_trials`` (which goes through the object) and ``nsof_accum_trials_c2c_dev`` (create, one step, read-outs and
    destroy over the caller's d_w) against the object stepped once."""
    import torch

    from nsof import _lib
    from nsof.accumulator import _frame_maps_c, accum_params, trial_param_maps_arg
    c = K.CASES[case]
    want = one_shot(nsof_lib, ctx, case, 5, N.NOISE)
    ev, idx = stream(case)
    maps = T.trial_maps(case, S.SEEDS)[0]
    got = nsof_lib.simulate_trials(ev, maps, c["version"], 1000, K.ACTIVE_V, c["silent_v"], c["polarity"], sensor_size=K.SMALL, params=K.PARAMS,
                                   dt=K.DT, refractory_us=c["refractory_us"], theta_events=c["theta"], snapshot_every=T.SNAP_EVERY,
                                   memsize=T.MEMSIZE, ctx=ctx, c2c=N.NOISE)
    assert same(got, want)
    n, planes = trial_param_maps_arg(maps, K.SMALL)
    dev = torch.device("cuda", ctx.device)
    out = dict(w=torch.empty(want["w"].shape, dtype=torch.float32, device=dev), resistance=torch.empty(want["w"].shape, dtype=torch.float32, device=dev),
               block_current=torch.empty(want["block_current"].shape, dtype=torch.float64, device=dev))
    torch.cuda.synchronize(dev)
    ap, nz = accum_params(K.PARAMS, K.DT, c["refractory_us"]), _lib.AccumC2c(*nsof_lib.c2c_arg(N.NOISE))
    split = int(c["version"] == 2 and c["polarity"] == "split")
    ctx.check(ctx._lib.nsof_accum_trials_c2c_dev(ctx.ptr, *K.SMALL, c["version"], split, K.ACTIVE_V, c["silent_v"], C.byref(ap), c["theta"],
                                                 *(a.ctypes.data for a in ev), idx.ctypes.data, S.N_SLICES, T.SNAP_EVERY, T.MEMSIZE, 1.0, n,
                                                 len(planes), *_frame_maps_c(n, planes), out["w"].data_ptr(), out["resistance"].data_ptr(),
                                                 out["block_current"].data_ptr(), C.byref(nz)), "trials_c2c_dev")
    assert same({k: v.cpu().numpy() for k, v in out.items()}, want)


def test_the_refractory_rule_straddles_the_cut(nsof_lib, ctx):
    """small_v2_split cut at k = 8: the restatement suppresses at least one pulse in slice 8 because of an earlier slice
    (next_ok must survive the cut), and the chunked run still equals the one-shot run -- which a run that forgot next_ok at
    the cut would not."""
    case = "small_v2_split"
    assert len(S.suppressed_after(case, 8)) >= 1
    want = one_shot(nsof_lib, ctx, case, 3, N.NOISE)
    assert same(run_chunks(nsof_lib, ctx, case, 3, (8,), N.NOISE), want)
    ev, idx = stream(case)
    acc = make(nsof_lib, ctx, case, 3, N.NOISE)
    try:
        first = acc.step(*ev, idx[:9])
        st = acc.state()
        assert st["next_ok"].shape == (2,) + K.SMALL and st["next_ok"].max() > ev[3][idx[8]]        # someone is still refractory
        acc.load_state(dict(w=st["w"], slice_counter=8))                                            # ... and now nobody is
        forgot = read(acc, [first, acc.step(*ev, idx[8:])])
    finally:
        acc.close()
    assert not np.array_equal(bits(forgot["w"]), bits(want["w"]))


@pytest.mark.parametrize("case", ["small_v1_theta3", "small_v2_split", "small_v1_mixed"])
def test_checkpoint_through_the_host(nsof_lib, ctx, case):
    want = one_shot(nsof_lib, ctx, case, 5, N.NOISE)
    ev, idx = stream(case)
    acc = make(nsof_lib, ctx, case, 5, N.NOISE)
    try:
        first = acc.step(*ev, idx[:21])
        st = acc.state()
    finally:
        acc.close()
    assert st["slice_counter"] == 20 and st["w"].shape == want["w"].shape and st["w"].dtype == F
    assert st["next_ok"].shape == want["w"].shape[:1] + K.SMALL and st["next_ok"].dtype == np.int64
    assert (st["next_ok"] != 0).any() == (K.CASES[case]["version"] == 2)
    with pytest.raises(nsof_lib.error, match="closed"):
        acc.step(*ev, idx[20:])
    acc = make(nsof_lib, ctx, case, 5, N.NOISE)
    try:
        for bad in (dict(st, w=st["w"][:, :4]), dict(st, w=st["w"][0]), dict(st, next_ok=st["next_ok"][..., :-1]), dict(st, slice_counter=-1)):
            with pytest.raises(nsof_lib.error):
                acc.load_state(bad)
        assert acc.slice_counter == 0
        acc.load_state(st)
        assert acc.slice_counter == 20
        got = read(acc, [first, acc.step(*ev, idx[20:])])
        assert acc.slice_counter == 40
    finally:
        acc.close()
    assert same(got, want)


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split", "small_v1_leak"])
def test_reset_gives_a_fresh_object(nsof_lib, ctx, case):
    want = one_shot(nsof_lib, ctx, case, 3, N.NOISE)
    ev, idx = stream(case)
    acc = make(nsof_lib, ctx, case, 3, N.NOISE)
    try:
        acc.step(*ev, idx[:14])
        acc.reset()
        assert acc.slice_counter == 0
        st = acc.state()
        assert np.array_equal(bits(st["w"][0]), bits(T.trial_maps(case, S.SEEDS[:3])[0]["wini"])) and not st["next_ok"].any()
        got = read(acc, [acc.step(*ev, idx)])
    finally:
        acc.close()
    assert same(got, want)


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
def test_block_currents_of_the_current_state(nsof_lib, ctx, case):
    """A chunk that ends on a snapshot slice (35): ``block_current_dev()`` is that snapshot.  Without ``memsize`` a step
    returns nothing and there are no block currents to read."""
    ev, idx = stream(case)
    acc = make(nsof_lib, ctx, case, 5, N.NOISE)
    try:
        cur = acc.step(*ev, idx[:37])
        now = acc.block_current_dev()
        ctx.synchronize()
        assert cur.shape[2] == 6 and tuple(now.shape) == tuple(cur.shape[:2]) + tuple(cur.shape[3:])
        assert np.array_equal(now.cpu().numpy().view(np.int64), cur[:, :, -1].cpu().numpy().view(np.int64))
        assert not np.array_equal(now.cpu().numpy(), cur[:, :, 0].cpu().numpy())
    finally:
        acc.close()
    acc = make(nsof_lib, ctx, case, 5, N.NOISE, memsize=None)
    try:
        assert acc.step(*ev, idx) is None and acc.slice_counter == S.N_SLICES
        with pytest.raises(nsof_lib.error, match="memsize"):
            acc.block_current_dev()
        w = acc.w_dev()
        ctx.synchronize()
        assert np.array_equal(bits(w.cpu().numpy()), bits(one_shot(nsof_lib, ctx, case, 5, N.NOISE)["w"]))
    finally:
        acc.close()


def assert_trial_equals(got, t, want, model, closest, label):
    for a, wk in enumerate(("w_final", "w_final_b")[: got["w"].shape[0]]):
        differ = int((bits(got["w"][a, t]) != bits(want[wk])).sum())
        print(f"{label} trial {t} {wk}: {differ} of {want[wk].size} states differ from the restatement (closest midpoint approach {closest:.3g})")
        if closest >= K.NEAR:
            assert differ == 0
        ulps = ulp_diff(got["resistance"][a, t], M.resistance_exp(got["w"][a, t], model))
        print(f"{label} trial {t} resistance of {wk}: at most {int(ulps.max())} ulp from the restatement's of the same state")
        assert (ulps <= 1).all()


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
def test_noise_identity_of_a_chunked_run(nsof_lib, ctx, case):
    got = run_chunks(nsof_lib, ctx, case, 5, S.THREE_CHUNKS, N.NOISE)
    for t, seed in enumerate(S.SEEDS):
        want, model, closest = N.restatement(case, seed, t, N.NOISE)
        assert_trial_equals(got, t, want, model, closest, case)


@pytest.mark.parametrize("noise", [None, S.VOLT_NOISE], ids=["quiet", "noise"])
@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
def test_a_write_voltage_per_trial(nsof_lib, ctx, case, noise):
    got = run_chunks(nsof_lib, ctx, case, 5, (20,), noise, active_v=S.ACTIVE_V)
    assert same(got, run_chunks(nsof_lib, ctx, case, 5, (), noise, active_v=np.float64(S.ACTIVE_V)))
    for t, v in enumerate(S.ACTIVE_V):
        want, model, closest = S.restatement(case, t, v, 0.0, S.items(noise or S.QUIET))
        assert_trial_equals(got, t, want, model, closest, f"{case} at {v} V")
    # trials 0 and 3 run at the case's own voltage: the scalar run's bits, with drive planes of their own
    base = run_chunks(nsof_lib, ctx, case, 5, (), noise)
    for t in (0, 3):
        assert all(np.array_equal(got[k][:, t].view(np.uint8), base[k][:, t].view(np.uint8)) for k in got), t
    assert all(not np.array_equal(bits(got["w"][:, t]), bits(base["w"][:, t])) for t in (1, 2, 4))


@pytest.mark.parametrize("noise", [None, S.VOLT_NOISE], ids=["quiet", "noise"])
def test_one_leaking_trial_puts_all_on_the_every_pixel_form(nsof_lib, ctx, noise):
    case = "small_v1"
    got = run_chunks(nsof_lib, ctx, case, 5, (20,), noise, silent_v=S.LEAK_SILENT_V)
    for t, sv in enumerate(S.LEAK_SILENT_V):
        want, model, closest = S.restatement(case, t, K.ACTIVE_V, sv, S.items(noise or S.QUIET))
        assert_trial_equals(got, t, want, model, closest, f"{case} silent at {sv} V")
    # the touched-pixels form (every trial idle at 0 V) against the every-pixel form, on the trials that do not leak
    zero = run_chunks(nsof_lib, ctx, case, 5, (20,), noise, silent_v=[0.0] * 5)
    for t in (0, 1, 3, 4):
        assert all(np.array_equal(got[k][:, t].view(np.uint8), zero[k][:, t].view(np.uint8)) for k in got), t
    assert not np.array_equal(bits(got["w"][:, 2]), bits(zero["w"][:, 2]))


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split", "small_v1_leak"])
def test_a_sequence_of_equal_voltages_is_the_scalar(nsof_lib, ctx, case):
    want = one_shot(nsof_lib, ctx, case, 5, N.NOISE)
    sv = K.CASES[case]["silent_v"]
    assert same(run_chunks(nsof_lib, ctx, case, 5, (8,), N.NOISE, active_v=[K.ACTIVE_V] * 5, silent_v=[sv] * 5), want)
    assert same(run_chunks(nsof_lib, ctx, case, 5, (), N.NOISE, active_v=[K.ACTIVE_V] * 5), want)
    assert same(run_chunks(nsof_lib, ctx, case, 5, (), N.NOISE, silent_v=tuple([sv] * 5)), want)


def single(nsof, ctx, case, planes, shape=K.SMALL):
    c = K.CASES[case]
    return nsof.Accumulator(*shape, c["version"], c["polarity"], K.ACTIVE_V, c["silent_v"], ctx=ctx, param_maps=planes, params=K.PARAMS, dt=K.DT,
                            refractory_us=c["refractory_us"], theta_events=c["theta"])


def assert_surfaces_equal(acc, singles, arrays, pad=0):
    """Every surface of the trial object against the single arrays' own, bit for bit; ``pad``: extra columns of the row."""
    import torch
    T_, H, W = acc.trials, acc.H, acc.W  # noqa: N806
    dev = torch.device("cuda", acc.ctx.device)
    for which in range(arrays):
        for mode in ("state", "current"):
            for dtype, mine, theirs in ((torch.uint8, acc.surface_u8_dev, "surface_u8"), (torch.float32, acc.surface_f32_dev, "surface_f32")):
                full = torch.full((T_, H, W + pad), 171, dtype=dtype, device=dev)
                got = mine(full[:, :, :W], which=which, mode=mode) if pad else mine(which=which, mode=mode)
                want = torch.empty((T_, H, W), dtype=dtype, device=dev)
                torch.cuda.synchronize(dev)
                for t, one in enumerate(singles):
                    getattr(one, theirs)(want[t], which=which, mode=mode)
                acc.ctx.synchronize()
                assert got.dtype == dtype and tuple(got.shape) == (T_, H, W)
                assert torch.equal(got.view(torch.uint8) if dtype == torch.uint8 else got.view(torch.int32),
                                   want.view(torch.uint8) if dtype == torch.uint8 else want.view(torch.int32)), (which, mode, dtype)
                if pad:
                    assert bool((full[:, :, W:] == 171).all()), "the padding was written"
                if mode == "state":
                    assert len(torch.unique(got)) > 10


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
def test_surfaces_equal_the_single_arrays(nsof_lib, ctx, case):
    ev, idx = stream(case)
    per = T.trial_maps(case, S.SEEDS)[1]
    arrays = 2 if case == "small_v2_split" else 1
    acc = make(nsof_lib, ctx, case, 5)
    singles = [single(nsof_lib, ctx, case, per[t]) for t in range(5)]
    try:
        for a, b in ((0, 20), (20, 40)):
            acc.step(*ev, idx[a:b + 1])
            for one in singles:
                one.step(*ev, idx[a:b + 1])
            assert_surfaces_equal(acc, singles, arrays)
        assert_surfaces_equal(acc, singles[:5], arrays, pad=11)          # rows of 48 values: the padding stays
        with pytest.raises(nsof_lib.error):
            acc.surface_u8_dev(which=arrays)
        import torch
        with pytest.raises(nsof_lib.error):
            acc.surface_f32_dev(torch.empty((5,) + K.SMALL, dtype=torch.uint8, device=torch.device("cuda", ctx.device)))
    finally:
        acc.close()
        for one in singles:
            one.close()


@pytest.mark.parametrize("pad", [0, 8, 1], ids=["dense", "padded-by-8", "padded-by-1"])
def test_surfaces_where_the_stores_are_vectorised(nsof_lib, ctx, pad):
    """A 6x40 sensor (W a multiple of 4) with states loaded through the host: dense rows and rows padded by 8 take the
    four-pixel stores, rows padded by 1 the pixel-by-pixel form; the same frames either way."""
    case, shape, trials = "small_v1", (6, 40), 3
    rng = np.random.default_rng(11)
    planes = [K.maps_of(shape, seed) for seed in S.SEEDS[:trials]]
    w = rng.random((1, trials) + shape, dtype=F)
    w[0, :, 0, :4] = F([0.0, 1.0, 0.42, 0.5])
    c = K.CASES[case]
    acc = nsof_lib.TrialAccumulator(*shape, {k: np.stack([m[k] for m in planes]) for k in planes[0]}, c["version"], c["polarity"], K.ACTIVE_V,
                                    c["silent_v"], params=K.PARAMS, dt=K.DT, ctx=ctx)
    singles = [single(nsof_lib, ctx, case, m, shape) for m in planes]
    try:
        acc.load_state(dict(w=w))
        for t, one in enumerate(singles):
            one.load_state(dict(w=w[0, t]))
        assert_surfaces_equal(acc, singles, 1, pad=pad)
    finally:
        acc.close()
        for one in singles:
            one.close()


def test_refusals_by_the_library(nsof_lib, ctx):
    from nsof import _lib
    from nsof.accumulator import accum_params
    H, W = K.SMALL  # noqa: N806
    ap = accum_params(K.PARAMS, K.DT, 20)

    def create(active, silent, trials=5):
        p = C.c_void_p()
        va, vs = F(active), F(silent)
        rc = ctx._lib.nsof_accum_trials_create(ctx.ptr, H, W, 1, 0, C.byref(ap), 1, trials, 0, None, None, None, None, va.ctypes.data, va.size,
                                               vs.ctypes.data, vs.size, 7, 3, 1.0, C.byref(p))
        return rc, p, ctx._lib.nsof_last_error(ctx.ptr).decode()

    for active, silent, words in (([-6.0, -4.0], [0.0], ("2 voltages", "5 trials")), ([-6.0], [0.0] * 4, ("4 voltages", "5 trials")),
                                  ([-6.0, -6.0, float("nan"), -6.0, -6.0], [0.0], ("active_v", "trial 2", "nan")),
                                  ([-6.0], [0.0, 0.0, 0.0, float("inf"), 0.0], ("silent_v", "trial 3", "inf")), ([float("nan")], [0.0], ("trial 0",))):
        rc, p, msg = create(active, silent)
        assert rc == _lib.NSOF_EINVAL and not p.value and all(w in msg for w in words), msg
    rc, p, _ = create([-6.0], [0.0])
    assert rc == _lib.NSOF_OK and p.value
    try:
        w = np.zeros((5, H, W), F)
        nok = np.zeros((2, H, W), np.int64)
        for n_w, n_ok, ok_ptr in ((4, 1, None), (6, 1, None), (5, 2, nok.ctypes.data)):
            assert ctx._lib.nsof_accum_trials_write_state(p, w.ctypes.data, n_w, ok_ptr, n_ok, 0) == _lib.NSOF_EINVAL
            assert "planes" in ctx._lib.nsof_last_error(ctx.ptr).decode()
        assert ctx._lib.nsof_accum_trials_write_state(p, w.ctypes.data, 5, None, 0, -1) == _lib.NSOF_EINVAL
        assert ctx._lib.nsof_accum_trials_write_state(p, w.ctypes.data, 5, nok.ctypes.data, 1, 3) == _lib.NSOF_OK
        cnt = C.c_int64()
        assert ctx._lib.nsof_accum_trials_read_state(p, None, None, C.byref(cnt)) == _lib.NSOF_OK and cnt.value == 3
        assert ctx._lib.nsof_accum_trials_snaps_in(p, 12) == 2                                   # slices 7 and 14 of 3 .. 14
        assert ctx._lib.nsof_accum_trials_step(p, None, None, None, None, nok.ctypes.data, 12, None, None) == _lib.NSOF_EINVAL
    finally:
        ctx._lib.nsof_accum_trials_destroy(p)


@pytest.mark.parametrize("case", ["small_v1", "small_v2_split"])
def test_a_refused_step_leaves_the_object_as_it_was(nsof_lib, ctx, case):
    want = one_shot(nsof_lib, ctx, case, 3, N.NOISE)
    ev, idx = stream(case)
    acc = make(nsof_lib, ctx, case, 3, N.NOISE)
    try:
        first = acc.step(*ev, idx[:21])
        before = acc.state()
        x = ev[0].copy()
        x[idx[30]] = K.SMALL[1]                                              # an event of chunk 2 outside the sensor
        with pytest.raises(nsof_lib.error, match="outside"):
            acc.step(x, *ev[1:], idx[20:])
        down = idx[20:].copy()
        down[3] = down[2] - 1
        with pytest.raises(nsof_lib.error, match="monotone"):
            acc.step(*ev, down)
        after = acc.state()
        assert after["slice_counter"] == before["slice_counter"] == 20
        assert np.array_equal(bits(after["w"]), bits(before["w"])) and np.array_equal(after["next_ok"], before["next_ok"])
        assert acc.step(*ev, idx[20:21]).shape[2] == 0                       # no slice: nothing happens
        got = read(acc, [first, acc.step(*ev, idx[20:])])
    finally:
        acc.close()
    assert same(got, want)
