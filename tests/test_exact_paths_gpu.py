"""Exact row-sum mode (NSOF_OPT_EXACT_ROWSUMS = 1, the default) equals the CPU oracle BIT FOR BIT on every dispatch path
nsof_farneback_core can take, through the pairs and the sequence entry points:

  * k_iterate_x (the fused strip walker): batches with NSOF_OPT_SMALL_BATCH_JOBS = 0;
  * the three-kernel small-batch form (farneback_iterate_lat.hip): lone calls and small batches at the default 64;
  * the unfused exact pair k_blur_colsum + k_blur_rowsolve: winsize > 15, iterations = 0, levels below 2x2;
  * the 64-pair recursion of that unfused path (sequences, batches above 64 pairs);
  * memory chunking (NSOF_MAX_PAIRS);

at the widths around the 192-column strips, the heights around the min_size 32 level truncation, 1xN / Nx1 frames,
strided views and the whole parameter range.  Plus the work-list edges: more than 256 overlapping crops pasted in
order, and an item wider than 255 strips inside a list."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A = (0.5, 3, 15, 3, 5, 1.2, 0)
B = (0.6, 3, 3, 3, 10, 1.05, 0)
Cc = (0.6, 3, 4, 2, 1, 1.05, 0)


def _frames(seed, n, h, w):
    """n frames of a sequence with motion between them (crops of one larger synthetic image)."""
    from nsof import synth
    base, _ = synth.make_pair(seed, h + 2 * n + 8, w + 3 * n + 8)
    return np.stack([np.ascontiguousarray(base[2 * i:2 * i + h, 3 * i:3 * i + w]) for i in range(n)])


def _diff(got, want):
    d = np.abs(got.astype(np.float64) - want)
    return f"max-abs {d.max():.3g}, {(got != want).sum()} of {got.size} values differ"


def _batch_and_sequence(nsof_lib, ctx, frames, params):
    """Flows of the consecutive pairs of `frames` through the device batch entry (prev and next apart) and the
    device sequence entry."""
    import torch
    n, h, w = frames.shape[0] - 1, frames.shape[1], frames.shape[2]
    P = nsof_lib.FarnebackParams(*params)
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(frames[:-1].copy()).to(dev)
    dn = torch.from_numpy(frames[1:].copy()).to(dev)
    ds = torch.from_numpy(frames).to(dev)
    fb = torch.empty((n, h, w, 2), dtype=torch.float32, device=dev)
    fs = torch.empty_like(fb)
    torch.cuda.synchronize()
    nsof_lib.farneback_batch(dp, dn, fb, n, h, w, P, ctx=ctx)
    nsof_lib.farneback_sequence(ds, fs, n + 1, h, w, P, ctx=ctx)
    ctx.synchronize()
    return fb.cpu().numpy(), fs.cpu().numpy()


def _check_all(nsof_lib, ctx, oracle, frames, params, tag):
    want = [oracle.farneback(frames[i], frames[i + 1], *params) for i in range(frames.shape[0] - 1)]
    got_b, got_s = _batch_and_sequence(nsof_lib, ctx, frames, params)
    for i, wt in enumerate(want):
        assert np.array_equal(got_b[i], wt), (tag, "batch", i, _diff(got_b[i], wt))
        assert np.array_equal(got_s[i], wt), (tag, "sequence", i, _diff(got_s[i], wt))
    one = nsof_lib.calcOpticalFlowFarneback(frames[0], frames[1], None, *params, ctx=ctx)
    assert np.array_equal(one, want[0]), (tag, "lone call", _diff(one, want[0]))


@pytest.fixture
def jobs(ctx):
    """Sets NSOF_OPT_SMALL_BATCH_JOBS for one test and restores the default."""
    from nsof import _lib
    assert ctx.get_option(_lib.OPT_EXACT_ROWSUMS) == 1
    assert ctx.get_option(_lib.OPT_SMALL_BATCH_JOBS) == 64
    try:
        yield lambda v: ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, v)
    finally:
        ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, 64)


# ---- the path matrix ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,params,n", [
    ("iterate_x", A, 3),                               # SMALL_BATCH_JOBS = 0: the fused strip walker
    ("small_batch", A, 2),                             # the default: the three-kernel form
    ("unfused_w16", (0.5, 2, 16, 2, 5, 1.1, 0), 3),    # winsize > 15: k_blur_colsum + k_blur_rowsolve
    ("unfused_w17", (0.5, 3, 17, 3, 5, 1.2, 0), 3),
    ("unfused_w21", (0.6, 2, 21, 2, 7, 1.5, 0), 2),
    ("unfused_w31", (0.5, 1, 31, 2, 5, 1.1, 0), 2),
    ("iterations0", (0.5, 3, 15, 0, 5, 1.2, 0), 2),
    ("levels0", (0.5, 0, 9, 3, 5, 1.1, 0), 3),
    ("levels0_small_batch", (0.5, 0, 5, 2, 7, 1.5, 0), 2),
])
def test_dispatch_paths_bit_identical(nsof_lib, ctx, oracle, jobs, path, params, n):
    jobs(0 if path in ("iterate_x", "levels0") else 64)
    _check_all(nsof_lib, ctx, oracle, _frames(17 + n, n + 1, 97, 203), params, path)


@pytest.mark.parametrize("winsize,max_pairs", [(17, None), (9, None), (17, "40")], ids=["17", "9", "17-max_pairs40"])
def test_more_than_64_pairs(nsof_lib, ctx, oracle, jobs, monkeypatch, winsize, max_pairs):
    """winsize 17: the unfused exact path runs batches above 64 pairs and every sequence in 64-pair chunks (a 65-pair
    batch, a 66-frame sequence); winsize 9: the same sizes through k_iterate_x.  NSOF_MAX_PAIRS=40: the 64-pair cap and the
    cap by hand both bind."""
    jobs(0)
    if max_pairs:
        monkeypatch.setenv("NSOF_MAX_PAIRS", max_pairs)
    params = (0.5, 2, winsize, 2, 5, 1.1, 0)
    frames = _frames(5, 66, 24, 40)
    want = [oracle.farneback(frames[i], frames[i + 1], *params) for i in range(65)]
    got_b, got_s = _batch_and_sequence(nsof_lib, ctx, frames, params)
    for i in range(65):
        assert np.array_equal(got_b[i], want[i]), ("batch", i, _diff(got_b[i], want[i]))
        assert np.array_equal(got_s[i], want[i]), ("sequence", i, _diff(got_s[i], want[i]))


@pytest.mark.parametrize("params", [A, (0.5, 2, 17, 2, 5, 1.1, 0)], ids=["fused", "unfused"])
@pytest.mark.parametrize("small_batch", [0, 64])
def test_memory_chunking_bit_identical(nsof_lib, ctx, oracle, jobs, monkeypatch, params, small_batch):
    """NSOF_MAX_PAIRS caps the pairs per chunk by hand: every chunk size gives the oracle's bits."""
    jobs(small_batch)
    frames = _frames(23, 6, 64, 200)
    want = [oracle.farneback(frames[i], frames[i + 1], *params) for i in range(5)]
    for cap in ("1", "2", "4"):
        monkeypatch.setenv("NSOF_MAX_PAIRS", cap)
        got_b, got_s = _batch_and_sequence(nsof_lib, ctx, frames, params)
        for i in range(5):
            assert np.array_equal(got_b[i], want[i]), (cap, "batch", i, _diff(got_b[i], want[i]))
            assert np.array_equal(got_s[i], want[i]), (cap, "sequence", i, _diff(got_s[i], want[i]))


# ---- shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(40, 191), (40, 192), (40, 193), (37, 383), (37, 384), (37, 385), (33, 961),
                                   (2, 200), (3, 200), (33, 150), (34, 150), (35, 37), (61, 97), (1, 50), (50, 1),
                                   (5, 3)])
@pytest.mark.parametrize("small_batch", [0, 64])
def test_edge_shapes_bit_identical(nsof_lib, ctx, oracle, jobs, shape, small_batch):
    """Strip and wave edges (widths around 192 and its multiples), the min_size 32 level truncation (heights 2, 3,
    33, 34), odd x odd, and frames whose levels fall below 2x2 (the unfused pair)."""
    jobs(small_batch)
    h, w = shape
    frames = _frames(h * 1000 + w, 3, h, w)
    for params in (A, Cc):
        _check_all(nsof_lib, ctx, oracle, frames, params, (shape, params))


def test_strided_views_bit_identical(nsof_lib, ctx, oracle, jobs):
    """Row-strided (non-contiguous) host views and a row stride on the device batch and sequence entries."""
    import torch
    big = _frames(41, 3, 230, 420)
    for small_batch in (0, 64):
        jobs(small_batch)
        for (y0, y1, x0, x1) in [(7, 207, 11, 398), (0, 35, 193, 386)]:
            pv, nv = big[0, y0:y1, x0:x1], big[1, y0:y1, x0:x1]
            assert not pv.flags.c_contiguous
            want = oracle.farneback(np.ascontiguousarray(pv), np.ascontiguousarray(nv), *A)
            got = nsof_lib.calcOpticalFlowFarneback(pv, nv, None, *A, ctx=ctx)
            assert np.array_equal(got, want), (small_batch, (y0, y1, x0, x1), _diff(got, want))
    # device entries with row_stride > width: the frames of `big`, cut to their first 300 columns
    h, w, rs = 230, 300, 420
    dev = torch.device("cuda", 0)
    P = nsof_lib.FarnebackParams(*B)
    want = [oracle.farneback(np.ascontiguousarray(big[i, :, :w]), np.ascontiguousarray(big[i + 1, :, :w]), *B) for i in range(2)]
    for small_batch in (0, 64):
        jobs(small_batch)
        d = torch.from_numpy(big).to(dev)
        fs = torch.empty((2, h, w, 2), dtype=torch.float32, device=dev)
        fb = torch.empty_like(fs)
        torch.cuda.synchronize()
        nsof_lib.farneback_sequence(d, fs, 3, h, w, P, row_stride=rs, ctx=ctx)
        nsof_lib.farneback_batch(d[:-1], d[1:], fb, 2, h, w, P, row_stride=rs, ctx=ctx)
        ctx.synchronize()
        for i in range(2):
            assert np.array_equal(fs[i].cpu().numpy(), want[i]), (small_batch, "sequence", i)
            assert np.array_equal(fb[i].cpu().numpy(), want[i]), (small_batch, "batch", i)


# ---- parameters --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poly_n", range(1, 11))
@pytest.mark.parametrize("poly_sigma", [0.0, 1.1])
def test_poly_n_sweep_bit_identical(nsof_lib, ctx, oracle, jobs, poly_n, poly_sigma):
    frames = _frames(poly_n, 3, 64, 96)
    for small_batch in (0, 64):
        jobs(small_batch)
        _check_all(nsof_lib, ctx, oracle, frames, (0.5, 2, 7, 2, poly_n, poly_sigma, 0), (poly_n, poly_sigma, small_batch))


@pytest.mark.parametrize("pyr_scale", [0.5, 0.6, 0.75, 0.8])
@pytest.mark.parametrize("params", [A, B, Cc], ids=["A", "B", "C"])
def test_pyr_scale_and_reference_sets_bit_identical(nsof_lib, ctx, oracle, jobs, pyr_scale, params):
    frames = _frames(int(pyr_scale * 100), 3, 120, 200)
    p = (pyr_scale,) + params[1:]
    for small_batch in (0, 64):
        jobs(small_batch)
        _check_all(nsof_lib, ctx, oracle, frames, p, (p, small_batch))


# ---- work-list edges ---------------------------------------------------------------------------------------------------
def test_crowded_paste_later_rectangle_wins(nsof_lib, ctx, oracle):
    """A crop with 299 later rectangles over it -- more than the paste kernel keeps in its LDS list (256).  Table of one
    frame: an anchor (in place), then a 600x40 crop that overlaps it (computed privately and pasted), then 299 crops
    of 4x8 px side by side on its top 16 rows: each covers a part of the big crop that no other rectangle covers, so a
    rectangle left out of the coverage test lets the big crop's paste write over the later crop's pixels.  The canvas
    must be the reference's loop -- every crop's flow pasted in table order, the later one wins -- on two calls."""
    import torch
    H, W = 48, 608
    frames = _frames(77, 2, H, W)
    table = [(590, 32, 600, 40), (0, 0, 600, 40)] + [(4 * (k % 150), 8 * (k // 150), 4 * (k % 150) + 4, 8 * (k // 150) + 8)
                                                     for k in range(299)]
    rects = np.zeros((2, len(table), 4), np.int32)
    rects[0] = table
    counts = np.array([len(table), 0], np.int32)
    params = nsof_lib.farneback.PARAMS_B
    pk = params.as_kwargs()
    p = tuple(pk[k] for k in ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags"))
    want = np.zeros((H, W, 2), np.float32)
    for x0, y0, x1, y1 in table:
        want[y0:y1, x0:x1] = oracle.farneback(np.ascontiguousarray(frames[0, y0:y1, x0:x1]),
                                              np.ascontiguousarray(frames[1, y0:y1, x0:x1]), *p)
    big = oracle.farneback(np.ascontiguousarray(frames[0, :40, :600]), np.ascontiguousarray(frames[1, :40, :600]), *p)
    assert (want[:16, :596] != big[:16, :596]).any(axis=-1).mean() > 0.9   # the pixels the later crops own tell them apart
    dev = torch.device("cuda", 0)
    d_frames, d_counts, d_rects = (torch.from_numpy(a).to(dev) for a in (frames, counts, rects))
    for call in range(2):
        flows = torch.full((1, H, W, 2), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        n_calls, _ = nsof_lib.farneback_roi_sequence_dev(d_frames, d_counts, d_rects, flows, params, gate_frame=0, ctx=ctx)
        ctx.synchronize()
        assert n_calls == len(table)
        got = flows[0].cpu().numpy()
        assert np.array_equal(got, want), (call, _diff(got, want))
    # a fresh context: a table of two crops (one paste), then the whole table -- its work-list and paste tables and the
    # private flow buffers grow while they hold the earlier call's data
    fresh = nsof_lib.Context(0)
    try:
        for n in (2, len(table)):
            d_counts = torch.tensor([n, 0], dtype=torch.int32, device=dev)
            flows = torch.full((1, H, W, 2), 7.0, dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            n_calls, _ = nsof_lib.farneback_roi_sequence_dev(d_frames, d_counts, d_rects, flows, params, gate_frame=0, ctx=fresh)
            fresh.synchronize()
            assert n_calls == n
        got = flows[0].cpu().numpy()
        assert np.array_equal(got, want), _diff(got, want)
    finally:
        fresh.close()


@pytest.mark.parametrize("exact", [1, 0])
def test_over_wide_item_in_work_list(nsof_lib, ctx, oracle, exact):
    """An item of 49 200 columns (256 strips of 192: above the 255 a k_iterate_x job can name) in a list with two small
    crops: every flow equals its per-call result (the oracle in exact mode; the lone call in fast mode)."""
    from nsof import _lib, synth
    wide_p, wide_n = synth.make_pair(3, 40, 49200)
    small_p, small_n = synth.make_pair(4, 120, 200)
    pairs = [(small_p[10:70, 5:150], small_n[10:70, 5:150]), (wide_p, wide_n), (small_p[50:, 60:], small_n[50:, 60:])]
    params = nsof_lib.farneback.PARAMS_A
    kw = params.as_kwargs()
    p = tuple(kw[k] for k in ("pyr_scale", "levels", "winsize", "iterations", "poly_n", "poly_sigma", "flags"))
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, exact)
    try:
        flows = nsof_lib.farneback_pairs(pairs, params, ctx=ctx)
        for i, (a, b) in enumerate(pairs):
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            want = oracle.farneback(a, b, *p) if exact else nsof_lib.calcOpticalFlowFarneback(a, b, None, *p, ctx=ctx)
            assert np.array_equal(flows[i], want), (exact, i, _diff(flows[i], want))
    finally:
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 1)
