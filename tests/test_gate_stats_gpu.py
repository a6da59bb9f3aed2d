"""GPU: gate statistics over the trials of a variability study (``nsof_gate_stats_dev``) against their NumPy statement
(``gating.gate_stats`` on ``gating.current_to_gray``), exactly; and the join ``pipeline.gating_variability_dev``."""
import numpy as np
import pytest

from test_frames_dev_gpu import _moving_patch_frames

pytestmark = pytest.mark.gpu

THRES, F = 245, 4
LO, HI = 4.75e-7, 3.8e-6      # log-uniform currents; the threshold current of gray 245, 7.8e-7 A, lies inside


def stats_case(trials, grid):
    """Currents of ``trials`` stacks and a nominal one, and their NumPy statistics."""
    from nsof import gating
    rng = np.random.default_rng(1000 * trials + grid[0] * grid[1])
    draw = lambda shape: np.exp(rng.uniform(np.log(LO), np.log(HI), shape))  # noqa: E731
    cur, nom = draw((trials, F) + grid), draw((F,) + grid)
    counts, flips = gating.gate_stats(cur, nom, THRES)
    return cur, nom, counts, flips


def check_preconditions(trials, counts, flips):
    """Some count strictly between 0 and T -- with one trial no count can be: there both 0 and 1 must occur -- and some flip."""
    if trials > 1:
        assert ((counts > 0) & (counts < trials)).any()
    else:
        assert (counts == 0).any() and (counts == 1).any()
    assert (flips > 0).any()


@pytest.mark.parametrize("grid", [(1, 1), (4, 4), (13, 24)])
@pytest.mark.parametrize("trials", [1, 5, 70])
def test_counts_and_flips_equal_numpy(nsof_lib, ctx, torch_dev, trials, grid):
    import torch
    from nsof import gating
    assert LO < 7.8e-7 < HI and gating.current_to_gray(7.9e-7) >= THRES > gating.current_to_gray(7.7e-7)
    cur, nom, counts, flips = stats_case(trials, grid)
    check_preconditions(trials, counts, flips)
    d_cur, d_nom = torch.from_numpy(cur).to(torch_dev), torch.from_numpy(nom).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    got_c, got_f = gating.gate_stats_dev(d_cur, d_nom, THRES, ctx=ctx)
    ctx.synchronize()
    assert got_c.dtype == torch.int32 and got_f.dtype == torch.int32
    assert got_c.shape == (F,) + grid and got_f.shape == (trials, F)
    assert np.array_equal(got_c.cpu().numpy(), counts)
    assert np.array_equal(got_f.cpu().numpy(), flips)
    # the gated bit is the byte roi_from_surface_dev writes
    cfg = gating.GatingConfig(MEMSIZE=1, THRES=THRES, OFFSET=0)
    _, _, gray = gating.roi_from_surface_dev(d_cur, trials * F, grid, grid, cfg, ctx=ctx, want_gray=True)
    ctx.synchronize()
    g = gray.cpu().numpy().reshape((trials, F) + grid)
    assert np.array_equal(g, gating.current_to_gray(cur))
    assert np.array_equal((g >= THRES).sum(axis=0), counts)


def test_gate_stats_refusals(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import _lib, gating
    cur = torch.ones((2, 3, 4, 4), dtype=torch.float64, device=torch_dev)
    nom = torch.ones((3, 4, 4), dtype=torch.float64, device=torch_dev)
    for a, b in ((cur.cpu(), nom), (cur.float(), nom), (cur, nom[:2]), (cur[0], nom), (cur[:, :, :, ::2], nom)):
        with pytest.raises(nsof_lib.error) as e:
            gating.gate_stats_dev(a, b, THRES, ctx=ctx)
        assert isinstance(e.value, ValueError)
    out = torch.full((64,), -7, dtype=torch.int32, device=torch_dev)
    lib = ctx._lib
    torch.cuda.synchronize(torch_dev)
    for args in ((None, nom.data_ptr(), 2, 3, 4, 4), (cur.data_ptr(), None, 2, 3, 4, 4), (cur.data_ptr(), nom.data_ptr(), 0, 3, 4, 4),
                 (cur.data_ptr(), nom.data_ptr(), 2, 0, 4, 4), (cur.data_ptr(), nom.data_ptr(), 2, 3, 0, 4)):
        assert lib.nsof_gate_stats_dev(ctx.ptr, *args, THRES, out.data_ptr(), out.data_ptr()) == _lib.NSOF_EINVAL
    assert lib.nsof_gate_stats_dev(ctx.ptr, cur.data_ptr(), nom.data_ptr(), 2, 3, 1 << 14, 1 << 14, THRES, out.data_ptr(),
                                   out.data_ptr()) == _lib.NSOF_EUNSUPPORTED
    ctx.synchronize()
    assert (out.cpu().numpy() == -7).all()


SPREAD = dict(koff=0.1, Ron=0.1)


def test_join_variability(nsof_lib, ctx, torch_dev):
    """8 frames of 96 x 128, MEMSIZE 16, n_sub_steps 20, 3 trials."""
    import torch
    from nsof import gating, pipeline
    cfg = gating.GatingConfig(MEMSIZE=16, THRES=THRES, OFFSET=0)
    d_bgr = torch.from_numpy(_moving_patch_frames()).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    nominal = pipeline.gating_stack_from_frames_dev(d_bgr, cfg, n_sub_steps=20, ctx=ctx)       # the path before maps
    T = 3  # noqa: N806
    # a spread of zero reproduces the nominal array in every trial, bit for bit
    zero = pipeline.gating_variability_dev(d_bgr, cfg, dict(koff=0.0, Ron=0.0), T, n_sub_steps=20, ctx=ctx)
    assert zero["stacks"].shape == (T, 7, 6, 8) and zero["stacks"].dtype == torch.float64
    assert torch.equal(zero["nominal"], nominal)
    for t in range(T):
        assert torch.equal(zero["stacks"][t], nominal), t
    assert int(zero["flips"].abs().sum()) == 0
    gated = torch.from_numpy(gating.current_to_gray(nominal.cpu().numpy()) >= THRES).to(torch_dev)
    assert torch.equal(zero["counts"], gated.to(torch.int32) * T)

    out = pipeline.gating_variability_dev(d_bgr, cfg, SPREAD, T, seed=3, n_sub_steps=20, ctx=ctx)
    assert set(out) >= {"nominal", "stacks", "p_gate", "flips", "counts", "rects"}
    assert torch.equal(out["nominal"], nominal)
    stacks = out["stacks"].cpu().numpy()
    counts, flips = gating.gate_stats(stacks, nominal.cpu().numpy(), THRES)
    print("flips per (trial, slice):", flips.tolist())
    assert np.array_equal(out["counts"].cpu().numpy(), counts) and np.array_equal(out["flips"].cpu().numpy(), flips)
    assert out["p_gate"].dtype == torch.float64 and np.array_equal(out["p_gate"].cpu().numpy(), counts / T)
    assert (flips > 0).any()                    # a 10 % spread on koff and Ron moves some cell across the threshold
    # trial t is the array run with the planes of seed 3 + t
    from nsof.accumulator import variability_maps
    maps1 = variability_maps(6, 8, SPREAD, None, seed=3 + 1, dtype=np.float64)
    one = pipeline.gating_stack_from_frames_dev(d_bgr, cfg, n_sub_steps=20, ctx=ctx, param_maps=maps1)
    assert one.shape == (1, 7, 6, 8) and torch.equal(one[0], out["stacks"][1])
    # rects[t] is the gating table of stacks[t]
    assert out["rects"].shape == (T, 7, 32, 4) and out["rect_counts"].shape == (T, 7)
    for t in range(T):
        c, r = gating.roi_from_surface_dev(out["stacks"][t], 7, (6, 8), (96, 128), cfg, max_rects=32, ctx=ctx)
        ctx.synchronize()
        assert torch.equal(out["rect_counts"][t], c)
        got, want = gating.rects_to_host(out["rect_counts"][t], out["rects"][t], ctx=ctx), gating.rects_to_host(c, r, ctx=ctx)
        assert got == want, t
    assert int(out["rect_counts"].sum()) > 0
    # a trial's stack is a mem_state of the sequence experiments, as it lies in HBM
    p_dev = pipeline.prediction_sequence_dev(d_bgr, out["stacks"][1], cfg, ctx=ctx)
    p_host = pipeline.prediction_sequence_dev(d_bgr, np.moveaxis(stacks[1], 0, 2), cfg, ctx=ctx)
    assert p_dev.keys() == p_host.keys()
    for key, v in p_host.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(p_dev[key], v), key
        else:
            assert p_dev[key] == v, key
    assert np.array_equal(out["stacks"].cpu().numpy(), stacks)          # read, not written
