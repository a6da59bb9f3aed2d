"""GPU: per-pixel parameter maps of the accumulator (nsof_accum_set_param_maps, ``Accumulator(param_maps=...)``).

Yardsticks: the uniform accumulator itself (constant planes must give its bits) and the NumPy restatement
tests/accum_maps_ref.py, whose contract is the device's applied per pixel.  The cases (tests/accum_maps_cases.py) keep every
power at least 2^-40 away from a float32 rounding midpoint (asserted in tests/test_accum_maps_cpu.py), so states are compared
bit for bit; resistances go through one more exp and are held to 1 ulp, as in tests/test_accum_params_gpu.py.  The stored
streams carry their own 48x64 sensor; the seeded one is 7x37 (259 pixels: quad tail, quads that straddle rows)."""
import ctypes as C
import gzip
import json

import numpy as np
import pytest

import accum_maps_cases as K  # noqa: N812
import accum_maps_ref as M  # noqa: N812
import accum_params_ref as R  # noqa: N812
from conftest import ulp_diff

pytestmark = pytest.mark.gpu

F = np.float32
VARIABILITY = [c for c in K.CASES if not K.CASES[c].get("mixed")]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def make(case, ctx, maps="case", **kw):
    """An accumulator of the case's scheme and scalars; ``maps``: "case" = the case's maps, None = the uniform device."""
    from nsof.accumulator import Accumulator
    c = K.CASES[case]
    _, (H, W) = K.stream_of(case)  # noqa: N806
    if maps == "case":
        maps = K.case_maps(case)
    return Accumulator(H, W, c["version"], c["polarity"], K.ACTIVE_V, c["silent_v"], ctx=ctx, params=K.PARAMS, dt=K.DT,
                       refractory_us=c["refractory_us"], theta_events=c["theta"], param_maps=maps, **kw)


def staged(acc, case):
    """Stage the stream of a case (or the event tuple given); -> its slice count."""
    from nsof.accumulator import slice_index_array
    ev = K.stream_of(case)[0] if isinstance(case, str) else case
    idx = slice_index_array(ev[3], 1000)
    acc.set_events(*ev, idx)
    return len(idx) - 1


def outputs(acc, case, torch_dev, snap_every=None):
    """Everything a run leaves: states, snapshots, the 8-bit surface in both modes, the float surface, the block current -- and
    the states of the same run without snapshots, whose groups are as long as the update form allows."""
    import torch
    n = staged(acc, case)
    acc.run(0, n, snap_every=max(1, n // 100) if snap_every is None else snap_every)
    out = dict(w=[acc.w(i) for i in range(2 if acc.split else 1)])
    out["block_snapshot"] = acc.block_current(3, snapshot=0)
    out["snaps"] = acc.snapshots()
    out["R"] = acc.resistance(0)
    for mode in ("state", "current"):
        u8 = torch.zeros((acc.H, acc.W), dtype=torch.uint8, device=torch_dev)
        f32 = torch.zeros((acc.H, acc.W), dtype=torch.float32, device=torch_dev)
        acc.surface_u8(u8, mode=mode)
        acc.surface_f32(f32, mode=mode)
        acc.ctx.synchronize()
        out["u8_" + mode], out["f32_" + mode] = u8.cpu().numpy(), f32.cpu().numpy()
    out["block"] = acc.block_current(3)
    acc.reset()
    acc.run(0, n)
    out["w_whole"] = [acc.w(i) for i in range(2 if acc.split else 1)]
    return out


CONSTANT = [(stream, mode) for stream in ("small", "golden") for mode in R.MODES]


@pytest.mark.parametrize("stream,mode", CONSTANT)
def test_constant_planes_give_the_uniform_accumulators_bits(nsof_lib, ctx, torch_dev, stream, mode):
    """All 13 keys mapped to constant planes of the scalars: w, the snapshots, both 8-bit surfaces, the float surface and the
    block current are those of the uniform accumulator, bit for bit."""
    from nsof.accumulator import Accumulator
    version, polarity, leak = R.MODES[mode]
    ev, (H, W) = K.small_stream() if stream == "small" else K.golden_stream(mode)  # noqa: N806
    maps = {k: np.full((H, W), K.PARAMS[k], F) for k in R.KEYS}
    got = []
    for pm in (None, maps):
        acc = Accumulator(H, W, version, polarity, K.ACTIVE_V, K.SET["leak_v"] if leak else 0.0, ctx=ctx, params=K.PARAMS, dt=K.DT,
                          refractory_us=K.SET["refractory_us"], param_maps=pm)
        try:
            assert set(acc.param_maps) == set(pm or {})
            got.append(outputs(acc, ev, torch_dev))
        finally:
            acc.close()
    uni, mapped = got
    assert len(np.unique(uni["w"][0])) > 10
    for i in range(len(uni["w"])):
        assert same_bits(uni["w"][i], mapped["w"][i]) and same_bits(uni["snaps"][i], mapped["snaps"][i]), i
        assert same_bits(uni["w"][i], uni["w_whole"][i]) and same_bits(uni["w"][i], mapped["w_whole"][i]), i
    assert uni["snaps"][0].shape[0] > 30
    for k in ("u8_state", "u8_current", "block", "block_snapshot"):
        assert np.array_equal(uni[k], mapped[k]), k
    for k in ("f32_state", "f32_current", "R"):
        assert same_bits(uni[k], mapped[k]), k


@pytest.mark.parametrize("dense", [True, False])
@pytest.mark.parametrize("case", VARIABILITY)
def test_variability_maps_equal_the_restatement(nsof_lib, ctx, torch_dev, case, dense):
    """10 % spread on kon, koff, von, voff, Ron, Roff, son, boff and a wini map, through the every-pixel pass and the
    event-pixel update (the leak case: the every-pixel pass with a per-pixel silent drive either way)."""
    want, model, _ = K.restatement(case)
    acc = make(case, ctx, dense=dense)
    try:
        got = outputs(acc, case, torch_dev)
    finally:
        acc.close()
    for i, (wk, rk) in enumerate((("w_final", "resistances"), ("w_final_b", "resistances_b"))[: len(got["w"])]):
        differ = int((bits(got["w"][i]) != bits(want[wk])).sum())
        print(f"{case} dense={dense} {wk}: {differ} of {want[wk].size} states differ from the restatement")
        assert differ == 0 and same_bits(got["w_whole"][i], want[wk])
        assert got["snaps"][i].shape == want[rk].shape and (ulp_diff(got["snaps"][i], want[rk]) <= 1).all()
    assert (ulp_diff(got["R"], M.resistance_exp(want["w_final"], model)) <= 1).all()
    for mode in ("state", "current"):
        assert np.array_equal(got["u8_" + mode], M.surface_u8(want["w_final"], model, mode)), mode
    assert same_bits(got["f32_state"], M.surface_f32(want["w_final"], model, "state"))
    # the current -> gray map in float: a resistance one ulp off (6e-8 relative) moves g = -3366 / log10(1 / R) - 306 by
    # 3366 * 6e-8 / (ln 10 * 5.2 ** 2) = 3e-6 at most (log10 R >= 5.2), and the result is rounded to float32 (ulp 1.5e-5 below 256)
    assert np.abs(got["f32_current"] - M.surface_f32(want["w_final"], model, "current")).max() <= 3e-6 + 2 * 1.6e-5
    H, W = got["R"].shape  # noqa: N806
    blocks = got["R"][: H // 3 * 3, : W // 3 * 3].reshape(H // 3, 3, W // 3, 3).min(axis=(1, 3))
    assert np.array_equal(got["block"], 1.0 / blocks.astype(np.float64))
    snap0 = got["snaps"][0][0][: H // 3 * 3, : W // 3 * 3].reshape(H // 3, 3, W // 3, 3).min(axis=(1, 3))
    assert np.array_equal(got["block_snapshot"], 1.0 / snap0.astype(np.float64))
    assert len(np.unique(got["u8_state"])) > 5


@pytest.mark.parametrize("case,every,n_frames", [("golden_v1", 8, 6), ("golden_v1", 70, 2), ("small_v1_theta3", 8, 5),
                                                   ("small_v1_leak", 8, 5)])
def test_variability_maps_through_the_frame_routes(nsof_lib, ctx, torch_dev, case, every, n_frames):
    """run_surface per interval and run_frames (every = 8: copy + patch whichever frames_path is set -- the tile walk has no
    mapped form; every = 70: n x run_surface) leave the restatement's states and the host map's frames."""
    import torch
    want, model, _ = K.restatement(case)
    states = [want["states"][every * (k + 1) - 1] for k in range(n_frames)]
    for mode in ("state", "current"):
        host = np.stack([M.surface_u8(s, model, mode) for s in states])
        if mode == "state":
            assert len(np.unique(host)) > 5 and (host[0] != host[-1]).any()
        results = {}

        def run(label, how, **kw):
            acc = make(case, ctx, **kw)
            frames = torch.zeros((n_frames, acc.H, acc.W), dtype=torch.uint8, device=torch_dev)
            try:
                staged(acc, case)
                how(acc, frames)
                ctx.synchronize()
                results[label] = (acc.w(0), frames.cpu().numpy())
            finally:
                acc.close()

        def fused(acc, frames):
            for k in range(n_frames):
                acc.run_surface(k * every, every, frames[k], mode=mode)

        def whole(acc, frames):
            acc.run_frames(0, n_frames, every, frames, mode=mode)

        run("run_surface", fused)
        run("run_surface, event-pixel update", fused, dense=False)
        run("run_frames", whole)
        run("run_frames copy_patch", whole, frames_path="copy_patch")
        run("run_frames, every-pixel pass", whole, dense=True)
        for label, (w, frames) in results.items():
            assert same_bits(w, states[-1]), (mode, label)
            assert np.array_equal(frames, host), (mode, label, int((frames != host).sum()))
        assert np.array_equal(results["run_frames"][1], results["run_frames copy_patch"][1])


@pytest.mark.parametrize("dense", [None, True, False])
def test_mixed_dead_zone_takes_the_every_pixel_pass(nsof_lib, ctx, torch_dev, dense):
    """silent_v = -0.3 with voff = -0.25 at half the pixels (they leak) and -0.35 at the others (they idle): the event-pixel
    update would skip the leaking pixels, so the library must not take it even when asked to (dense=False)."""
    case = "small_v1_mixed"
    want, model, _ = K.restatement(case)
    acc = make(case, ctx, dense=dense)
    try:
        got = outputs(acc, case, torch_dev)
    finally:
        acc.close()
    assert same_bits(got["w"][0], want["w_final"]), int((bits(got["w"][0]) != bits(want["w_final"])).sum())
    assert same_bits(got["w_whole"][0], want["w_final"])
    assert (ulp_diff(got["snaps"][0], want["resistances"]) <= 1).all()
    ev, (H, W) = K.stream_of(case)  # noqa: N806
    idle = np.ones((H, W), bool)
    idle[ev[1], ev[0]] = False
    leaks = K.case_maps(case)["voff"] > F(-0.3)
    wini = K.case_maps(case)["wini"]
    assert (idle & leaks).sum() >= 5 and (got["w"][0][idle & leaks] != wini[idle & leaks]).all()
    assert (idle & ~leaks).sum() >= 5 and same_bits(got["w"][0][idle & ~leaks], wini[idle & ~leaks])


def test_wini_map_reset_and_state_round_trip(nsof_lib, ctx):
    case = "small_v2_split"
    want, _, _ = K.restatement(case)
    wini = K.case_maps(case)["wini"]
    assert len(np.unique(wini)) > 100
    acc, other = make(case, ctx), make(case, ctx)
    try:
        assert same_bits(acc.w(0), wini) and same_bits(acc.w(1), wini)
        n = staged(acc, case)
        acc.run(0, n, snap_every=3)
        assert same_bits(acc.w(0), want["w_final"]) and acc.snapshot_count() > 0
        acc.reset()
        st = acc.state(0)
        assert same_bits(st["w"], wini) and same_bits(acc.w(1), wini) and st["slice_counter"] == 0 and not st["next_ok"].any()
        assert acc.snapshot_count() == 0
        # half a run, its state carried to another mapped accumulator, the rest there
        acc.run(0, n // 2)
        assert staged(other, case) == n
        for which in (0, 1):
            other.load_state(acc.state(which), which)
        other.run(n // 2, n - n // 2)
        assert same_bits(other.w(0), want["w_final"]) and same_bits(other.w(1), want["w_final_b"])
        assert other.state(0)["slice_counter"] == n
    finally:
        acc.close()
        other.close()


def test_refused_calls_leave_model_and_state(nsof_lib, ctx):
    """Every refusal is NSOF_EINVAL and changes nothing: the run that follows is the uniform accumulator's."""
    from nsof import _lib
    case = "small_v1"
    _, (H, W) = K.stream_of(case)  # noqa: N806
    lib = ctx._lib
    good = K.case_maps(case)
    uniform = make(case, ctx, maps=None)
    acc = make(case, ctx, maps=None)
    try:
        n = staged(uniform, case)
        uniform.run(0, n)
        want = uniform.w(0)
        staged(acc, case)

        def refused(maps, match):
            with pytest.raises(nsof_lib.error, match=match) as e:
                acc.set_param_maps(maps)
            assert e.value.status == _lib.NSOF_EINVAL
            assert acc.param_maps == {}

        von = good["von"].copy()
        von[3, 5] = -0.0
        refused(dict(good, von=von), r"von.*row 3, column 5")
        von[3, 5] = -0.125
        refused({"von": von}, r"von.*row 3, column 5.*-0\.125")
        ron = good["Ron"].copy()
        ron[6, 36] = 0.0
        refused({"Ron": ron, "Roff": good["Roff"]}, r"Ron.*row 6, column 36")
        son = np.full((H, W), 0.5, F)
        son[0, 0] = 1.5
        refused({"son": son}, r"son.*row 0, column 0")

        def raw(keys, planes):
            rc = lib.nsof_accum_set_param_maps(acc._p, len(keys), (C.c_int * len(keys))(*keys), (C.c_void_p * len(planes))(*planes))
            assert acc.param_maps == {}
            return rc, lib.nsof_last_error(ctx.ptr).decode()

        koff = good["koff"].copy()
        koff[2, 1] = np.nan
        rc, msg = raw([4], [koff.ctypes.data])
        assert rc == _lib.NSOF_EINVAL and "koff" in msg and "row 2, column 1" in msg
        rc, msg = raw([5, 5], [good["kon"].ctypes.data, good["kon"].ctypes.data])
        assert rc == _lib.NSOF_EINVAL and "kon" in msg and "twice" in msg
        assert raw([13], [good["kon"].ctypes.data])[0] == _lib.NSOF_EINVAL
        assert raw([-1], [good["kon"].ctypes.data])[0] == _lib.NSOF_EINVAL
        assert raw([5], [None])[0] == _lib.NSOF_EINVAL
        assert lib.nsof_accum_read_param_map(acc._p, 5, np.empty((H, W), F).ctypes.data) == _lib.NSOF_EINVAL
        assert same_bits(acc.w(0), np.full((H, W), K.PARAMS["wini"], F))
        # an accumulator that has advanced refuses maps, and goes on as the device it was
        acc.run(0, n // 2)
        half = acc.w(0)
        refused(good, "advanced")
        assert same_bits(acc.w(0), half)
        acc.run(n // 2, n - n // 2)
        assert same_bits(acc.w(0), want)
    finally:
        acc.close()
        uniform.close()


def test_round_trip_and_clearing(nsof_lib, ctx):
    case = "small_v1"
    want, _, _ = K.restatement(case)
    maps = K.case_maps(case)
    uniform, acc = make(case, ctx, maps=None), make(case, ctx)
    try:
        back = acc.param_maps
        assert list(back) == [k for k in R.KEYS if k in maps] and all(same_bits(back[k], maps[k]) for k in maps)
        n = staged(acc, case)
        staged(uniform, case)
        acc.run(0, n)
        uniform.run(0, n)
        assert same_bits(acc.w(0), want["w_final"]) and not same_bits(acc.w(0), uniform.w(0))
        # after a reset: another set of maps, then none
        acc.reset()
        acc.set_param_maps({"wini": maps["wini"]})
        assert list(acc.param_maps) == ["wini"] and same_bits(acc.w(0), maps["wini"])
        acc.set_param_maps(None)
        assert acc.param_maps == {} and same_bits(acc.w(0), np.full_like(maps["wini"], K.PARAMS["wini"]))
        acc.run(0, n)
        assert same_bits(acc.w(0), uniform.w(0))
        assert acc.params == uniform.params
    finally:
        acc.close()
        uniform.close()


def test_simulate_with_param_maps(nsof_lib, ctx, tmp_path):
    case = "small_v2_split"
    c = K.CASES[case]
    want, _, _ = K.restatement(case)
    ev, shape = K.stream_of(case)
    maps = K.case_maps(case)
    kw = dict(version=2, active_v=K.ACTIVE_V, polarity="split", sensor_size=shape, ctx=ctx, params=K.PARAMS, dt=K.DT,
              refractory_us=c["refractory_us"])
    out = nsof_lib.simulate(ev, param_maps=maps, out_prefix=tmp_path / "mapped", **kw)
    for k in ("w_final", "w_final_b"):
        assert same_bits(out[k], want[k]), k
    assert (ulp_diff(out["resistances"], want["resistances"]) <= 1).all()
    assert (ulp_diff(out["resistances_b"], want["resistances_b"]) <= 1).all()
    acc = make(case, ctx)
    try:
        n = staged(acc, case)
        acc.run(0, n, snap_every=max(1, n // 100))
        assert same_bits(acc.w(0), out["w_final"]) and same_bits(acc.w(1), out["w_final_b"])
        assert same_bits(acc.snapshots()[0], out["resistances"])
    finally:
        acc.close()
    z = np.load(tmp_path / "mapped.V2.npz")
    assert sorted(z.files) == sorted(["w_final", "resistances"] + [f"map_{k}" for k in maps])
    assert all(same_bits(z[f"map_{k}"], maps[k]) for k in maps) and same_bits(z["w_final"], out["w_final"])
    with gzip.open(tmp_path / "mapped.V2.json.gz", "rt") as fp:
        meta = json.load(fp)
    assert meta["param_maps"] == [k for k in R.KEYS if k in maps] and meta["params"]["kon"] == K.PARAMS["kon"]
    # without maps: the files the uniform run always wrote
    plain = nsof_lib.simulate(ev, out_prefix=tmp_path / "plain", **kw)
    assert not same_bits(plain["w_final"], out["w_final"])
    assert sorted(np.load(tmp_path / "plain.V2.npz").files) == ["resistances", "w_final"]
    with gzip.open(tmp_path / "plain.V2.json.gz", "rt") as fp:
        assert "param_maps" not in json.load(fp)
