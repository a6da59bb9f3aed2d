"""Shape-heterogeneous batches (nsof_farneback_u8_batch*) and the multi-dataset harness (BASELINE config 4).

CPU part: the call list the harness derives from the reference's own gating data (tests/golden/gating_stacks.npz =
data/*/constructed_3D_matrix.mat in full) and its round-robin sharding (gloo, world size 2).
GPU part: every call of a work list equals the per-call path bit for bit and the CPU oracle to 1e-5 px, for ROI
crops (strided views, unaligned origins) and full frames of the five datasets' real sizes and parameter sets.
"""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, PKG, ROOT

A = (0.5, 3, 15, 3, 5, 1.2, 0)


@pytest.fixture(scope="module")
def stacks():
    with np.load(os.path.join(GOLDEN, "gating_stacks.npz")) as z:
        return {k: z[k] for k in z.files}


def _small_frames(wl, stacks, n_pairs):
    return {name: wl.synthetic_sequence(7 + k, n_pairs + 1, *wl.DATASET_FRAMES[name][:2])
            for k, name in enumerate(stacks)}


# ---------------------------------------------------------------------------------------------------------------
# CPU: call list and sharding
# ---------------------------------------------------------------------------------------------------------------
def test_call_list_matches_reference_rectangles(nsof_lib, stacks):
    """ROI rectangles of the first pairs equal those SURVEY.md section 8f derived from the same .mat files, the
    call list has one full-frame call per pair, and ROI flows are views of the pair's canvas."""
    from nsof import workload as wl
    calls, canvases = wl.mixed_workload(stacks, pairs_per_dataset=3, frames=_small_frames(wl, stacks, 3))
    by = {}
    for c in calls:
        by.setdefault((c.dataset, c.kind), []).append(c)
    assert [c.rect for c in by[("grasp", "roi")]][:3] == [(460, 0, 1060, 1920), (300, 0, 1060, 1140),
                                                          (540, 940, 1060, 1140)]
    assert [c.rect for c in by[("tabletennis", "roi")]][:2] == [(0, 0, 160, 160), (70, 10, 160, 160)]
    # uavnew2 is FLAG 1 (one call per component); its union boxes are the rectangles SURVEY lists
    from nsof import gating
    cfg2 = gating.dataset_config("uavnew2", FLAG=2)
    merged = [wl.roi_rects(gating.gating_maps(stacks["uavnew2"], i, cfg2)[1], (600, 600), cfg2) for i in range(2)]
    assert merged == [[(0, 60, 600, 600)], [(180, 100, 420, 340)]]
    per_comp = [c.rect for c in by[("uavnew2", "roi")] if c.pair == 2]
    assert per_comp == [(220, 100, 380, 260), (260, 140, 420, 300), (220, 180, 380, 340)]
    for name in stacks:
        assert len(by[(name, "full")]) == 3 and len(canvases[name]) == 3
        for c in by.get((name, "roi"), []):
            x0, y0, x1, y1 = c.rect
            assert c.prev.shape == (y1 - y0, x1 - x0) == c.flow.shape[:2]
            assert np.shares_memory(c.flow if c.paste_to is None else c.paste_to, canvases[name][c.pair])
    # uavnew2 pair 0 has overlapping component boxes: private fields, pasted in order afterwards
    assert all(c.paste_to is not None for c in by[("uavnew2", "roi")] if c.pair == 0)
    assert all(c.paste_to is None for c in by[("grasp", "roi")])
    # parameter sets follow data/*/Parameters.txt
    from nsof.farneback import PARAMS_A, PARAMS_B, PARAMS_C
    want = {"grasp": PARAMS_A, "uavnew2": PARAMS_A, "autodriving": PARAMS_B, "uav": PARAMS_B, "tabletennis": PARAMS_C}
    assert all(c.params == want[c.dataset] for c in calls)


def test_full_workload_counts(nsof_lib, stacks):
    """All consecutive pairs of the five sequences: 99+98+98+46+19 full-frame
    calls; frames are not needed to count calls, so 2-frame stand-ins are tiled."""
    from nsof import gating
    from nsof import workload as wl
    n_full = n_roi = 0
    for name, (h, w, n_frames) in wl.DATASET_FRAMES.items():
        cfg = gating.dataset_config(name)
        n = min(n_frames - 2, stacks[name].shape[2] - cfg.OFFSET)
        for i in range(n):
            n_roi += len(wl.roi_rects(gating.gating_maps(stacks[name], i, cfg)[1], (h, w), cfg))
        n_full += n
    assert n_full == 99 + 98 + 98 + 46 + 19
    assert n_roi > 200


def test_roi_from_surface_c_abi_matches_python_gating(nsof_lib, stacks):
    """nsof_roi_from_surface (the C export SURVEY 8b suggests) against the Python mirror of opticalFlow3D's gating on
    EVERY slice of the reference's five constructed_3D_matrix.mat stacks, both FLAG settings, connectivity 4 and 8."""
    from nsof import gating
    from nsof import workload as wl
    n = 0
    for name, (h, w, _) in wl.DATASET_FRAMES.items():
        for flag in (1, 2):
            for conn in (4, 8):
                cfg = gating.dataset_config(name, FLAG=flag, CONNECT=conn)
                for k in range(stacks[name].shape[2]):
                    sl = stacks[name][:, :, k]
                    want = wl.roi_rects(gating.current_to_gray(sl), (h, w), cfg)
                    got = gating.roi_from_surface(sl, (h, w), cfg)
                    assert [r for r in got if r[2] > r[0] and r[3] > r[1]] == want, (name, flag, conn, k)
                    n += len(got)
    assert n > 1000


def _fake_pairs(pairs, params, flows):
    for (p, q), f in zip(pairs, flows):
        f[..., 0] = p.astype(np.float32) - q
        f[..., 1] = float(params.winsize)


def _shard_worker(rank, world, port, ret):
    for p_ in (ROOT, PKG):
        if p_ not in sys.path:
            sys.path.insert(0, p_)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from nsof import dist as nd
    from nsof import workload as wl
    nd.init_from_env("gloo")
    with np.load(os.path.join(GOLDEN, "gating_stacks.npz")) as z:
        st = {k: z[k] for k in ("uav", "tabletennis")}
    frames = {name: wl.synthetic_sequence(3 + k, 5, *wl.DATASET_FRAMES[name][:2]) for k, name in enumerate(st)}
    calls, _ = wl.mixed_workload(st, pairs_per_dataset=4, frames=frames)
    mine = wl.shard_calls(calls, rank, world)
    wl.run_calls(mine, pairs_fn=_fake_pairs)
    sums = [(i, float(c.flow.astype(np.float64).sum())) for i, c in zip(range(rank, len(calls), world), mine)]
    gathered = [None] * world if rank == 0 else None
    dist.gather_object(sums, gathered, dst=0)
    t = nd.max_over_ranks(1.0 + rank)
    if rank == 0:
        wl.run_calls(calls, pairs_fn=_fake_pairs)           # unsharded reference
        want = {i: float(c.flow.astype(np.float64).sum()) for i, c in enumerate(calls)}
        got = {i: s for part in gathered for i, s in part}
        ret.put(bool(got == want and t == float(world) and len(got) == len(calls)))
    dist.barrier()
    dist.destroy_process_group()


def test_round_robin_world2():
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ret = ctx.Queue()
    port = 29700 + (os.getpid() % 100)
    procs = [ctx.Process(target=_shard_worker, args=(r, 2, port, ret)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    assert ret.get(timeout=5) is True


# ---------------------------------------------------------------------------------------------------------------
# GPU: work list == per call == oracle
# ---------------------------------------------------------------------------------------------------------------
def _crops(seed, shapes, frame_hw=(700, 900)):
    """Strided ROI views of one big frame pair at unaligned origins."""
    from nsof import synth
    prev, nxt = synth.make_pair(seed, *frame_hw)
    rng = np.random.default_rng(seed)
    out = []
    for (h, w) in shapes:
        y0 = int(rng.integers(0, frame_hw[0] - h + 1))
        x0 = int(rng.integers(0, frame_hw[1] - w + 1))
        out.append((prev[y0:y0 + h, x0:x0 + w], nxt[y0:y0 + h, x0:x0 + w]))
    return out


SHAPES = [(200, 520), (131, 97), (64, 64), (33, 70), (300, 301), (48, 200), (520, 200), (40, 40), (2, 2), (1, 9),
          (161, 161), (256, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("params", [A, (0.6, 3, 3, 3, 10, 1.05, 0), (0.6, 3, 4, 2, 1, 1.05, 0), (0.75, 5, 8, 1, 3, 0.9, 0)])
def test_work_list_equals_per_call(nsof_lib, ctx, params):
    nsof = nsof_lib
    p = nsof.FarnebackParams(*params)
    pairs = _crops(11, SHAPES)
    got = nsof.farneback_pairs(pairs, p, ctx=ctx)
    for (a, b), g in zip(pairs, got):
        want = nsof.calcOpticalFlowFarneback(a, b, None, **p.as_kwargs(), ctx=ctx)
        assert g.shape == want.shape and g.dtype == np.float32
        assert np.array_equal(g, want), (a.shape, float(np.abs(g - want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("small_batch_jobs", [None, 1 << 20])
def test_skewed_work_list_equals_per_call(nsof_lib, ctx, small_batch_jobs):
    """One full frame among hundreds of small crops (what gating produces on a sparse stream): the level tables are
    sorted into size classes with a launch each and the fused kernel takes its (item, strip) jobs from per-XCD lists
    of the strips that exist -- every flow must still equal the lone call's.  small_batch_jobs=2^20: the same list
    through the three-kernel small-batch form (whole-level grids over the sorted tables)."""
    nsof = nsof_lib
    from nsof import _lib
    p = nsof.FarnebackParams(*A)
    rng = np.random.default_rng(77)
    shapes = [(720, 1280), (300, 400), (17, 500), (410, 33), (500, 17)]
    shapes += [(int(rng.integers(40, 90)), int(rng.integers(40, 90))) for _ in range(260)]
    shapes += [(int(rng.integers(100, 260)), int(rng.integers(100, 400))) for _ in range(24)]
    order = rng.permutation(len(shapes))
    shapes = [shapes[i] for i in order]
    pairs = _crops(13, shapes, frame_hw=(720, 1280))
    if small_batch_jobs is not None:
        old = ctx.get_option(_lib.OPT_SMALL_BATCH_JOBS)
        ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, small_batch_jobs)
    try:
        got = nsof.farneback_pairs(pairs, p, ctx=ctx)
    finally:
        if small_batch_jobs is not None:
            ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, old)
    for (a, b), g in zip(pairs, got):
        want = nsof.calcOpticalFlowFarneback(a, b, None, **p.as_kwargs(), ctx=ctx)
        assert np.array_equal(g, want), (a.shape, float(np.abs(g - want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("params", [A, (0.6, 3, 3, 3, 10, 1.05, 0), (0.6, 3, 4, 2, 1, 1.05, 0), (0.5, 2, 9, 2, 7, 1.5, 0)])
def test_small_item_lists_equal_per_call(nsof_lib, ctx, params):
    """Two hundred small items (2..140 rows, 2..140 columns: strips a third full, jobs of a few steps, several size
    classes) in one list, four parameter sets: every flow equal to the lone call's."""
    nsof = nsof_lib
    p = nsof.FarnebackParams(*params)
    rng = np.random.default_rng(5)
    shapes = [(64, 64), (65, 65), (63, 200), (200, 63), (9, 64), (300, 64), (128, 128), (129, 127), (2, 2), (3, 64), (64, 3)]
    shapes += [(int(rng.integers(2, 140)), int(rng.integers(2, 70))) for _ in range(150)]
    shapes += [(int(rng.integers(20, 200)), int(rng.integers(60, 140))) for _ in range(40)]
    pairs = _crops(17, shapes, frame_hw=(400, 500))
    got = nsof.farneback_pairs(pairs, p, ctx=ctx)
    for (a, b), g in zip(pairs, got):
        want = nsof.calcOpticalFlowFarneback(a, b, None, **p.as_kwargs(), ctx=ctx)
        assert np.array_equal(g, want), (a.shape, float(np.abs(g - want).max()))


@pytest.mark.gpu
def test_work_list_vs_oracle_and_canvas_paste(nsof_lib, ctx, oracle):
    """ROI flows written in place into frame-sized canvases (the paste of optical_flow_seg.py:162/204), pinned and
    pageable targets, several pipeline chunks; compared with the CPU oracle."""
    nsof = nsof_lib
    p = nsof.FarnebackParams(*A)
    pairs = _crops(5, SHAPES[:8])
    canvases = [np.zeros((600, 640, 2), np.float32) for _ in pairs]
    flows = [c[7:7 + a.shape[0], 3:3 + a.shape[1]] for c, (a, _) in zip(canvases, pairs)]
    os.environ["NSOF_PIPE_CHUNK_MB"] = "1"            # ~1 MiB of flow per chunk: the list takes several chunks
    try:
        nsof.farneback_pairs(pairs, p, flows, ctx=ctx)
        pinned = nsof.farneback_pairs(pairs, p, pinned=True, ctx=ctx)
    finally:
        del os.environ["NSOF_PIPE_CHUNK_MB"]
    for (a, b), f, c, pf in zip(pairs, flows, canvases, pinned):
        ref = oracle.farneback(np.ascontiguousarray(a), np.ascontiguousarray(b), *A)
        assert float(np.abs(f - ref).max()) <= 1e-5
        assert np.array_equal(pf, f)
        outside = c.copy()
        outside[7:7 + a.shape[0], 3:3 + a.shape[1]] = 0
        assert not outside.any()                       # nothing outside the ROI was touched


@pytest.mark.gpu
def test_pipelined_entry_drains_on_error(nsof_lib, ctx, oracle):
    """An error in the middle of the pipelined host entry (injected after chunk 1 of several, NSOF_PIPE_FAIL_AFTER_CHUNK)
    must not leave uploads / downloads in flight: the call raises, the caller's arrays can be dropped at once, and the
    next call on the same context works and is correct."""
    from nsof.errors import NsofError
    nsof = nsof_lib
    p = nsof.FarnebackParams(*A)
    pairs = _crops(9, SHAPES[:8])
    os.environ["NSOF_PIPE_CHUNK_MB"] = "1"
    os.environ["NSOF_PIPE_FAIL_AFTER_CHUNK"] = "1"
    try:
        with pytest.raises(NsofError, match="injected failure"):
            nsof.farneback_pairs(pairs, p, ctx=ctx)
    finally:
        del os.environ["NSOF_PIPE_FAIL_AFTER_CHUNK"]
    try:
        got = nsof.farneback_pairs(pairs, p, ctx=ctx)
    finally:
        del os.environ["NSOF_PIPE_CHUNK_MB"]
    for (a, b), f in zip(pairs, got):
        assert np.array_equal(f, oracle.farneback(np.ascontiguousarray(a), np.ascontiguousarray(b), *A))


# Eleven items in eight chunks at NSOF_PIPE_CHUNK_MB=1 (a chunk closes once it holds >= 1 MiB of flow, so an item of at
# least 256x512 ends its chunk and smaller ones ride along with the next large one).  The pipeline has three slots: every
# slot is reused at least once, chunks 6 and 7 reuse one for the second time, and chunks 3..7 are larger than the chunk
# their slot held before, so the slot's buffers grow on reuse.
DEEP_CHUNKS = [[(256, 512)], [(40, 40), (256, 512)], [(256, 512)], [(264, 512)], [(33, 70), (2, 2), (272, 512)],
               [(280, 520)], [(288, 520)], [(256, 512)]]


@pytest.fixture(scope="module")
def deep_list(nsof_lib, ctx):
    """The crops of DEEP_CHUNKS (strided views of one 300x560 pair) and the lone call's flow of each."""
    p = nsof_lib.FarnebackParams(*A)
    pairs = _crops(23, [s for chunk in DEEP_CHUNKS for s in chunk], frame_hw=(300, 560))
    want = [nsof_lib.calcOpticalFlowFarneback(a, b, None, **p.as_kwargs(), ctx=ctx) for a, b in pairs]
    for w in want:
        w.setflags(write=False)
    return pairs, want


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement", ["pageable", "pinned", "mixed"])
def test_pipeline_slot_reuse_growth_and_mixed_memory(nsof_lib, deep_list, capfd, arrangement):
    """The pipelined host entry over eight chunks on a fresh context (empty slots): slot reuse two rounds deep, slot
    buffers that must grow, and frames / flows that are all pageable (strided crops, strided views into zeroed canvases),
    all page-locked, or mixed item by item (prev page-locked for even i, next for i % 3 == 0, flow for odd i: chunks
    mixed on both sides next to single-item chunks wholly of one kind).  Every flow equals the lone call's bit for bit;
    the mixed run also reads the chunk count from the library's own NSOF_PIPE_TRACE output."""
    nsof = nsof_lib
    from nsof.farneback import pinned_empty
    p = nsof.FarnebackParams(*A)
    pairs, want = deep_list
    assert len(pairs) == 11

    def locked(a):
        out = pinned_empty(a.shape, a.dtype)
        out[...] = a
        return out

    def lock_prev(i):
        return arrangement == "pinned" or (arrangement == "mixed" and i % 2 == 0)

    def lock_next(i):
        return arrangement == "pinned" or (arrangement == "mixed" and i % 3 == 0)

    def lock_flow(i):
        return arrangement == "pinned" or (arrangement == "mixed" and i % 2 == 1)

    frames = [(locked(a) if lock_prev(i) else a, locked(b) if lock_next(i) else b) for i, (a, b) in enumerate(pairs)]
    canvases = {i: np.zeros((a.shape[0] + 9, a.shape[1] + 5, 2), np.float32)
                for i, (a, _) in enumerate(pairs) if not lock_flow(i)}
    flows = [pinned_empty(a.shape + (2,), np.float32) if lock_flow(i) else canvases[i][7:7 + a.shape[0], 3:3 + a.shape[1]]
             for i, (a, _) in enumerate(pairs)]
    env = {"NSOF_PIPE_CHUNK_MB": "1"}
    if arrangement == "mixed":
        env["NSOF_PIPE_TRACE"] = "1"
    own = nsof.Context(0)   # a context whose slots are empty: their buffers have to grow
    capfd.readouterr()
    os.environ.update(env)
    try:
        nsof.farneback_pairs(frames, p, flows, ctx=own)
    finally:
        for k in env:
            del os.environ[k]
        own.close()
    err = capfd.readouterr().err
    if arrangement == "mixed":
        import re
        m = re.search(r"\[nsof pipe\] (\d+) chunks", err)
        assert m, err
        assert int(m.group(1)) == len(DEEP_CHUNKS) == 8
    for i, (f, w) in enumerate(zip(flows, want)):
        assert np.array_equal(f, w), (arrangement, i, f.shape, float(np.abs(f - w).max()))
    for i, c in canvases.items():
        h, w = pairs[i][0].shape
        outside = c.copy()
        outside[7:7 + h, 3:3 + w] = 0
        assert not outside.any(), (arrangement, i)      # nothing outside the view was written


@pytest.mark.gpu
def test_work_list_device_crops(nsof_lib, ctx, torch_dev):
    """Device-resident twin: crops of frames already in HBM, flows into crops of a device canvas."""
    import torch
    nsof = nsof_lib
    from nsof import synth
    p = nsof.FarnebackParams(*A)
    prev, nxt = synth.make_pair(21, 480, 640)
    dp, dn = torch.from_numpy(prev).to(torch_dev), torch.from_numpy(nxt).to(torch_dev)
    canvas = torch.zeros((480, 640, 2), dtype=torch.float32, device=torch_dev)
    full = torch.empty((480, 640, 2), dtype=torch.float32, device=torch_dev)
    rects = [(17, 33, 217, 293), (300, 100, 631, 431), (0, 0, 640, 480)]
    torch.cuda.synchronize()
    pairs = [(dp[y0:y1, x0:x1], dn[y0:y1, x0:x1]) for x0, y0, x1, y1 in rects]
    flows = [canvas[y0:y1, x0:x1] for x0, y0, x1, y1 in rects[:2]] + [full]
    nsof.farneback_pairs_dev(pairs, flows, p, ctx=ctx)
    ctx.synchronize()
    for (x0, y0, x1, y1), f in zip(rects, flows):
        want = nsof.calcOpticalFlowFarneback(prev[y0:y1, x0:x1], nxt[y0:y1, x0:x1], None, **p.as_kwargs(), ctx=ctx)
        assert np.array_equal(f.cpu().numpy(), want)


@pytest.mark.gpu
def test_config4_mixed_datasets_vs_oracle(nsof_lib, ctx, oracle, stacks):
    """BASELINE config 4 on one GPU: grasp + autodriving + uav + uavnew2 + tabletennis, each with its
    Parameters.txt, gated (ROI) and full-frame calls, frames of the real sizes; every flow vs the CPU oracle."""
    from nsof import workload as wl
    calls, canvases = wl.mixed_workload(stacks, pairs_per_dataset=2)
    assert {c.dataset for c in calls} == set(wl.DATASET_FRAMES) and {c.kind for c in calls} == {"roi", "full"}
    wl.run_calls(calls, ctx=ctx)
    worst = 0.0
    for c in calls:
        ref = oracle.farneback(np.ascontiguousarray(c.prev), np.ascontiguousarray(c.next),
                               *[getattr(c.params, k) for k in ("pyr_scale", "levels", "winsize", "iterations",
                                                                "poly_n", "poly_sigma", "flags")])
        worst = max(worst, float(np.abs(c.flow - ref).max()))
    assert worst <= 1e-5, worst
    # the one-call-at-a-time pattern of the reference gives the same bits
    again, canvases2 = wl.mixed_workload(stacks, pairs_per_dataset=2)
    wl.run_calls_one_by_one(again, ctx=ctx)
    assert all(np.array_equal(a.flow, b.flow) for a, b in zip(calls, again))
    # ... and the same canvases, overlapping component boxes included (later components win)
    for name in canvases:
        assert all(np.array_equal(a, b) for a, b in zip(canvases[name], canvases2[name])), name


@pytest.mark.gpu
def test_real_frames_through_harness(nsof_lib, ctx, oracle, stacks):
    """The reference's own first frames (tests/golden/frames/*, demo/grasp_*.jpg) through the gated + full-frame
    calls with each dataset's parameters, vs the oracle -- the 801x801 autodriving frames included."""
    pil = pytest.importorskip("PIL.Image")
    from nsof import gating
    from nsof import workload as wl

    def load(paths):
        out = []
        for pth in paths:
            bgr = np.ascontiguousarray(np.asarray(pil.open(pth).convert("RGB"))[..., ::-1])
            out.append(gating.frame_to_gray(bgr, "RGB2GRAY"))
        return out

    frames = {"grasp": load([os.path.join(GOLDEN, "demo", f"grasp_{k}.jpg") for k in (1, 2)])}
    for name in ("autodriving", "uav", "uavnew2", "tabletennis"):
        d = os.path.join(GOLDEN, "frames", name)
        frames[name] = load([os.path.join(d, f) for f in sorted(os.listdir(d), key=lambda s: int(s.split(".")[0]))])
    for name, fr in frames.items():
        assert fr[0].shape == wl.DATASET_FRAMES[name][:2]
    calls, _ = wl.mixed_workload(stacks, frames=frames, pairs_per_dataset=2)
    wl.run_calls(calls, ctx=ctx)
    # REAL frames, default mode: every stage keeps the reference's operation order, the box-filter row sums included (one
    # running sum per image row, carried from strip to strip inside the fused iteration kernel) -> bit-identical to the
    # oracle.  (Round 2's default summed each pixel's window directly: 80 of 641 601 pixels of the first autodriving pair
    # then moved by more than 1e-4, max 7.8e-4, because rank-deficient 3x3 windows amplify the sums' last bits; that is
    # now the opt-in fast mode, see test_fast_rowsum_mode_deviates_where_documented.)
    for c in calls:
        ref = oracle.farneback(np.ascontiguousarray(c.prev), np.ascontiguousarray(c.next),
                               *[getattr(c.params, k) for k in ("pyr_scale", "levels", "winsize", "iterations",
                                                                "poly_n", "poly_sigma", "flags")])
        assert np.array_equal(c.flow, ref), (c.dataset, c.kind, c.rect, float(np.abs(c.flow - ref).max()))


@pytest.mark.gpu
def test_roi_batch_is_cheaper_than_one_by_one(nsof_lib, ctx, torch_dev):
    """64 ROI pairs of 520x200 (the typical grasp crop) in one work list: well under 0.1 ms per pair on the device
    (one at a time: ~0.95 ms each)."""
    import time

    import torch
    nsof = nsof_lib
    p = nsof.FarnebackParams(*A)
    g = torch.Generator(device=torch_dev).manual_seed(0)
    frames = torch.randint(0, 256, (2, 1080, 1920), dtype=torch.uint8, device=torch_dev, generator=g)
    canvas = torch.zeros((64, 200, 520, 2), dtype=torch.float32, device=torch_dev)
    pairs = [(frames[0, 8 * i:8 * i + 200, 13 * i:13 * i + 520], frames[1, 8 * i:8 * i + 200, 13 * i:13 * i + 520])
             for i in range(64)]
    flows = [canvas[i] for i in range(64)]
    torch.cuda.synchronize()
    for _ in range(2):
        nsof.farneback_pairs_dev(pairs, flows, p, ctx=ctx)
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(5):
        nsof.farneback_pairs_dev(pairs, flows, p, ctx=ctx)
    ctx.synchronize()
    per_pair_ms = (time.perf_counter() - t0) / 5 / 64 * 1e3
    assert per_pair_ms < 0.1, per_pair_ms


@pytest.mark.gpu
def test_exact_rowsum_order_equals_oracle_on_real_frames(nsof_lib, ctx, oracle, stacks):
    """Default mode (NSOF_OPT_EXACT_ROWSUMS = 1): with the box-filter row sums formed in the library's order (one running
    sum per image row) the HIP path equals the CPU oracle BIT FOR BIT on the reference's real frames -- the 801x801
    autodriving pairs with the 3x3 window of parameter set B, where per-pixel window sums differ by up to 7.8e-4 at 80
    pixels -- through the per-call entry, the uniform batch / sequence and the work list."""
    pil = pytest.importorskip("PIL.Image")
    import torch
    from nsof import _lib, gating
    nsof = nsof_lib
    d = os.path.join(GOLDEN, "frames", "autodriving")
    fr = [gating.frame_to_gray(np.ascontiguousarray(np.asarray(pil.open(os.path.join(d, f"{k}.jpg")).convert("RGB"))[..., ::-1]),
                               "RGB2GRAY") for k in (1, 2, 3)]
    B = (0.6, 3, 3, 3, 10, 1.05, 0)
    p = nsof.FarnebackParams(*B)
    refs = [oracle.farneback(fr[i], fr[i + 1], *B) for i in range(2)]
    assert ctx.get_option(_lib.OPT_EXACT_ROWSUMS) == 1
    one = nsof.calcOpticalFlowFarneback(fr[0], fr[1], None, *B, ctx=ctx)
    lst = nsof.farneback_pairs([(fr[0], fr[1]), (fr[1], fr[2]), (fr[0][100:400, 50:700], fr[1][100:400, 50:700])], p, ctx=ctx)
    dev = torch.device("cuda", 0)
    frames = torch.from_numpy(np.stack(fr)).to(dev)
    flows = torch.empty((2, 801, 801, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    nsof.farneback_sequence(frames, flows, 3, 801, 801, p, ctx=ctx)
    ctx.synchronize()
    assert np.array_equal(one, refs[0])
    assert np.array_equal(lst[0], refs[0]) and np.array_equal(lst[1], refs[1])
    assert np.array_equal(lst[2], oracle.farneback(np.ascontiguousarray(fr[0][100:400, 50:700]),
                                                   np.ascontiguousarray(fr[1][100:400, 50:700]), *B))
    assert np.array_equal(flows.cpu().numpy(), np.stack(refs))
    # parameter set A on a synthetic pair
    from nsof import synth
    a, b = synth.make_pair(3, 270, 480)
    assert np.array_equal(nsof.calcOpticalFlowFarneback(a, b, None, *A, ctx=ctx), oracle.farneback(a, b, *A))


@pytest.mark.gpu
def test_fast_rowsum_mode_deviates_where_documented(nsof_lib, ctx, oracle):
    """NSOF_OPT_EXACT_ROWSUMS = 0 (opt-in fast mode: each pixel's window summed directly): within 1e-5 of the oracle on
    textured frames, and above 1e-4 (below 2e-3) on the real autodriving pair with parameter set B -- the deviation
    DESIGN.md section 2 documents; per call through the exact= keyword, which restores the context's setting."""
    pil = pytest.importorskip("PIL.Image")
    from nsof import _lib, gating, synth
    nsof = nsof_lib
    d = os.path.join(GOLDEN, "frames", "autodriving")
    fr = [gating.frame_to_gray(np.ascontiguousarray(np.asarray(pil.open(os.path.join(d, f"{k}.jpg")).convert("RGB"))[..., ::-1]),
                               "RGB2GRAY") for k in (1, 2)]
    B = (0.6, 3, 3, 3, 10, 1.05, 0)
    ref = oracle.farneback(fr[0], fr[1], *B)
    fast = nsof.calcOpticalFlowFarneback(fr[0], fr[1], None, *B, ctx=ctx, exact=False)
    assert ctx.get_option(_lib.OPT_EXACT_ROWSUMS) == 1                      # restored
    assert 1e-4 < float(np.abs(fast - ref).max()) < 2e-3
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 0)
    try:
        a, b = synth.make_pair(3, 270, 480)
        assert float(np.abs(nsof.calcOpticalFlowFarneback(a, b, None, *A, ctx=ctx) - oracle.farneback(a, b, *A)).max()) <= 1e-5
        assert np.array_equal(nsof.calcOpticalFlowFarneback(fr[0], fr[1], None, *B, ctx=ctx, exact=True), ref)
        assert ctx.get_option(_lib.OPT_EXACT_ROWSUMS) == 0
    finally:
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 1)
