"""The segmentation experiment of optical_flow_seg.py (__main__ :399-632, task_results :253-320) over a sequence.

CPU: both new entries are exported and bound, and the boxes ``pipeline.segmentation_sequence_dev`` segments are the
boxes ``run_segmentation`` hands its ``mask_fn`` (FLAG 2, FLAG 1, FLAG 1 merged), with the CPU oracle as flow backend.
GPU: the batched head (``nsof_motion_mask_sequence_dev``) against ``nsof_motion_mask_dev`` and ``oracle.motion_mask``
applied box by box onto a zeroed canvas, the batched pixel accuracy (``nsof_pixel_accuracy_u8_batch_dev``) against
``calculate_pixel_accuracy``, and ``segmentation_sequence_dev`` against ``run_segmentation`` with the GPU backends.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_path

SMALL = dict(MEMSIZE=16, EXTEND_HEIGHT_UPPER=4, EXTEND_HEIGHT_LOWER=4, EXTEND_WIDTH_LEFT=4, EXTEND_WIDTH_RIGHT=4)
DATASETS = ["autodriving", "uav", "uavnew2", "tabletennis"]


def _json_stack(name, keys):
    g = json.load(open(golden_path("gating_maps.json")))[name]
    return np.stack([np.array([[float(v) for v in row] for row in g["slices"][k]]) for k in keys], -1)


def _synthetic_bgr(seed, n, h, w):
    from nsof import workload as wl
    return [np.ascontiguousarray(np.repeat(f[..., None], 3, 2)) for f in wl.synthetic_sequence(seed, n, h, w)]


def _synthetic_gt(seed, n, h, w):
    """Ground-truth frames whose gray values straddle 127 (and so differ between channels in a way BGR2GRAY weighs)."""
    rng = np.random.default_rng(seed)
    gts = []
    for _ in range(n):
        g = rng.integers(100, 156, (h, w, 3), dtype=np.uint8)
        y0, x0 = int(rng.integers(0, h // 2)), int(rng.integers(0, w // 2))
        g[y0:y0 + h // 3, x0:x0 + w // 3] = 255
        gts.append(g)
    return gts


def _gt_binary(gt_bgr):
    from nsof import gating
    return np.where(gating.frame_to_gray(gt_bgr, "BGR2GRAY") > 127, np.uint8(255), np.uint8(0))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_entries_exported_and_bound(nsof_lib):
    from nsof import _lib
    lib = _lib.load()
    for name in ("nsof_motion_mask_sequence_dev", "nsof_pixel_accuracy_u8_batch_dev"):
        assert name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    for name in ("motion_mask_sequence_dev", "pixel_accuracy_batch_dev", "segmentation_sequence_dev"):
        assert callable(getattr(nsof_lib, name))


@pytest.mark.parametrize("flag,merge", [(2, False), (1, False), (1, True)])
def test_sequence_boxes_are_the_harness_boxes(nsof_lib, oracle, monkeypatch, flag, merge):
    """Every box ``run_segmentation`` segments, recovered from its crops (the Mem flow canvas is replaced by one that
    encodes each pixel's position), equals ``segmentation_sequence_dev``'s box list for the same rectangles."""
    from nsof import gating, pipeline
    stack = _json_stack("grasp", ("0", "1", "2", "3"))
    hm, wm = stack.shape[:2]
    h, w = hm * 16, wm * 16
    cfg = nsof_lib.dataset_config("grasp", FLAG=flag, **SMALL)
    frames = _synthetic_bgr(3, 5, h, w)
    gts = _synthetic_gt(4, 5, h, w)
    yy, xx = np.mgrid[0:h, 0:w]
    code = -np.stack([xx + 0.5, yy + 0.5], -1)       # run_segmentation negates: crop[0, 0] = (x0 + .5, y0 + .5)
    real = gating.opticalFlow3D
    rects, seen, state = [], [], {"in3d": False, "orig": False}

    def of3d(*a, **kw):
        state["in3d"] = True
        out = list(real(*a, **kw))
        state["in3d"] = False
        rs = list(out[5]) if flag == 1 else ([tuple(out[4])] if tuple(out[4]) != (0, 0, 0, 0) else [])
        rects.append([tuple(int(v) for v in r) for r in rs])
        seen.append([])
        out[0] = code
        return tuple(out)

    def flow(a, b, _f, **kw):
        if not state["in3d"]:
            state["orig"] = True                     # the full-frame flow: the next mask is the Original's
        return oracle.farneback(a, b, **kw)

    def mask(crop):
        if state["orig"]:
            state["orig"] = False
            assert crop.shape[:2] == (h, w)
        else:
            x0, y0 = int(crop[0, 0, 0] - 0.5), int(crop[0, 0, 1] - 0.5)
            seen[-1].append((x0, y0, x0 + crop.shape[1], y0 + crop.shape[0]))
        return np.zeros(crop.shape[:2], np.uint8)

    monkeypatch.setattr(gating, "opticalFlow3D", of3d)
    rows, _, _ = pipeline.run_segmentation(frames, gts, stack, cfg, merge_flag=merge, flow_fn=flow, mask_fn=mask)
    assert len(rows) == 3 and len(seen) == 3
    want = pipeline._experiment_boxes(rects, cfg, merge, (h, w))
    assert seen == [[b for b in bs if b[2] > b[0] and b[3] > b[1]] for bs in want]
    assert any(seen)                                 # the stacks gate something
    if flag == 1 and merge:
        assert all(len(b) <= 1 for b in seen)


# ---------------------------------------------------------------------------------------------------------------- GPU
def _per_box(nsof_lib, ctx, flows, boxes, **kw):
    """The per-box composition on the host canvas: ``nsof_motion_mask_dev`` of each crop, pasted in order."""
    import torch
    n, h, w = flows.shape[:3]
    out = np.zeros((n, h, w), np.uint8)
    for k in range(n):
        for x0, y0, x1, y1 in (boxes[k] if boxes is not None else [(0, 0, w, h)]):
            if x1 <= x0 or y1 <= y0:
                continue
            crop = flows[k, y0:y1, x0:x1].contiguous()
            m = torch.empty((y1 - y0, x1 - x0), dtype=torch.uint8, device=flows.device)
            torch.cuda.synchronize()
            nsof_lib.segment.motion_mask_dev(crop, m, y1 - y0, x1 - x0, ctx=ctx, **kw)
            ctx.synchronize()
            out[k, y0:y1, x0:x1] = m.cpu().numpy()
    return out


def _per_box_oracle(oracle, flows, boxes, seg_th=1, ksize=10, iterations=5):
    n, h, w = flows.shape[:3]
    out = np.zeros((n, h, w), np.uint8)
    for k in range(n):
        for x0, y0, x1, y1 in (boxes[k] if boxes is not None else [(0, 0, w, h)]):
            if x1 > x0 and y1 > y0:
                out[k, y0:y1, x0:x1] = oracle.motion_mask(flows[k, y0:y1, x0:x1], seg_th, ksize, iterations)
    return out


def _random_flows(torch_dev, seed, n, h, w):
    import torch
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((n, h, w, 2), generator=g) * 0.8            # |flow| straddles 1: speckled masks
    f[:, h // 4:h // 2, w // 5:w // 2] *= 4.0                    # a moving block
    return f.to(torch_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_mask_sequence_equals_per_box_composition(nsof_lib, ctx, oracle, torch_dev, iterations):
    from nsof import segment
    n, h, w = 6, 97, 131                                          # width not a multiple of 32 or 64
    flows = _random_flows(torch_dev, 5, n, h, w)
    boxes = [[(10, 5, 70, 50), (40, 20, 120, 90), (55, 30, 60, 35)],          # overlaps: the later box wins
             [(0, 0, 30, h), (w - 17, 0, w, 40), (0, h - 9, w, h), (0, 0, w, 1)],   # frame edges, a 1-px-tall box
             [],                                                               # no box
             [(5, 5, 5, 40), (20, 30, 60, 30), (64, 0, 65, h), (3, 3, 100, 90)],    # empty boxes, 1-px-wide box
             [(0, 0, w, h)],
             [(100, 60, 131, 97), (90, 50, 131, 97)]]
    got = segment.motion_mask_sequence_dev(flows, boxes, iterations=iterations, ctx=ctx)
    ctx.synchronize()
    got = got.cpu().numpy()
    want = _per_box(nsof_lib, ctx, flows, boxes, iterations=iterations)
    assert np.array_equal(got, want)
    assert np.array_equal(got, _per_box_oracle(oracle, flows.cpu().numpy(), boxes, iterations=iterations))
    assert not got[2].any()
    assert got.any() and (got != 0).sum() < got.size


@pytest.mark.gpu
def test_mask_sequence_many_overlapping_boxes_and_long_reach(nsof_lib, ctx, oracle, torch_dev):
    from nsof import segment
    n, h, w = 3, 120, 200
    flows = _random_flows(torch_dev, 9, n, h, w)
    rng = np.random.default_rng(1)
    many = []
    for _ in range(300):                                            # > 256 mutually overlapping boxes in one pair
        x0, y0 = int(rng.integers(0, 60)), int(rng.integers(0, 40))
        many.append((x0, y0, x0 + int(rng.integers(80, 140)), y0 + int(rng.integers(60, 80))))
    boxes = [many, [(0, 0, w, h)], [(7, 9, 150, 111)]]
    got = segment.motion_mask_sequence_dev(flows, boxes, ctx=ctx)
    ctx.synchronize()
    assert np.array_equal(got.cpu().numpy(), _per_box(nsof_lib, ctx, flows, boxes))
    # a fresh context: one box, then the 302 -- its box / job table grows while it holds the earlier call's data
    fresh = nsof_lib.Context(0)
    try:
        segment.motion_mask_sequence_dev(flows, [[(7, 9, 150, 111)], [], []], ctx=fresh)
        again = segment.motion_mask_sequence_dev(flows, boxes, ctx=fresh)
        fresh.synchronize()
        assert np.array_equal(again.cpu().numpy(), got.cpu().numpy())
    finally:
        fresh.close()
    # ksize 31: the element's reach splits the chain into several launches
    got = segment.motion_mask_sequence_dev(flows, boxes[1:] + [[(3, 2, 190, 118), (50, 40, 90, 80)]], ksize=31,
                                           iterations=3, ctx=ctx)
    ctx.synchronize()
    fl = flows.cpu().numpy()
    bx = boxes[1:] + [[(3, 2, 190, 118), (50, 40, 90, 80)]]
    assert np.array_equal(got.cpu().numpy(), _per_box(nsof_lib, ctx, flows, bx, ksize=31, iterations=3))
    assert np.array_equal(got.cpu().numpy(), _per_box_oracle(oracle, fl, bx, ksize=31, iterations=3))


def _sparse_flows(torch_dev, seed, n, h, w, scale):
    """Flows whose mask a closing neither empties nor fills: speckle of ``scale`` (rarely above 1), a block four times
    as strong that straddles 1, and a lattice of vectors of magnitude exactly 1 (which `mag > 1` leaves unset)."""
    import torch
    g = torch.Generator().manual_seed(seed)
    f = torch.randn((n, h, w, 2), generator=g) * scale
    f[:, h // 4:h // 2, w // 5:w // 2] *= 4.0
    f[:, ::7, ::5] = torch.tensor([1.0, 0.0])
    f[:, 3::7, 2::5] = torch.tensor([0.0, -1.0])
    return f.to(torch_dev)


def _check_both_entries(nsof_lib, ctx, oracle, flows, boxes, **kw):
    """The sequence entry against the single-image entry and the oracle, both applied box by box."""
    from nsof import segment
    got = segment.motion_mask_sequence_dev(flows, boxes, ctx=ctx, **kw)
    ctx.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got, _per_box(nsof_lib, ctx, flows, boxes, **kw))
    assert np.array_equal(got, _per_box_oracle(oracle, flows.cpu().numpy(), boxes, **kw))
    return got


@pytest.mark.gpu
def test_fixed_element_chain_of_two_launches_across_tiles(nsof_lib, ctx, oracle, torch_dev):
    """ksize 10, iterations 7: 14 passes of reach 5, while the 64-pixel halo holds 12, so plan_chunk gives launches of
    12 and 2 passes; 70 x 400 px is 3 tile rows of 32 and 2 tiles of 384 px.  cv2 does not reflect the even-sized
    element, so the sixth and seventh iteration differ (the oracle shows it) and reading the wrong bit image would too."""
    h, w = 70, 400
    flows = _sparse_flows(torch_dev, 11, 3, h, w, 0.35)
    boxes = [[(0, 0, w, h)], [(0, 0, w, h)], [(3, 2, 397, 66), (150, 20, 391, 70)]]   # x1 = 397, 391: inside a word
    got = _check_both_entries(nsof_lib, ctx, oracle, flows, boxes, ksize=10, iterations=7)
    assert all(0 < (m != 0).sum() < m.size for m in got[:2])
    whole = _check_both_entries(nsof_lib, ctx, oracle, flows[:1], None, ksize=10, iterations=7)
    assert np.array_equal(whole[0], got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(37, 53), (40, 450)])
def test_run_time_element_on_both_entries(nsof_lib, ctx, oracle, torch_dev, hw):
    """ksize 9 is not the fixed 10 x 10 ellipse: the arm that reads the element from the kernel argument."""
    h, w = hw
    flows = _sparse_flows(torch_dev, 12, 2, h, w, 0.35)
    got = _check_both_entries(nsof_lib, ctx, oracle, flows, [[(0, 0, w, h)], [(1, 2, w - 3, h - 1), (w // 3, 0, w, h // 2)]],
                              ksize=9, iterations=2)
    assert 0 < (got[0] != 0).sum() < got[0].size


@pytest.mark.gpu
@pytest.mark.parametrize("ksize,iterations", [(31, 1), (31, 2), (31, 3), (31, 4), (15, 5)])
def test_job_list_chain_result_buffer_parity(nsof_lib, ctx, oracle, torch_dev, ksize, iterations):
    """k_mask_compose must read the bit image the chain's last launch wrote.
    ksize 31 (reach 15, 10 distinct rows): plan_chunk allows min(64 / 15, passes left) = up to 4 passes per launch
    (tile of 32 + 4 * 30 = 152 rows, 11 * 152 * 64 B = 107008 B of LDS, above the 64 KB default and below the 144 KB
    budget), so iterations 1, 2, 3, 4 (2, 4, 6, 8 passes) take 1, 1, 2, 2 launches and leave the result in bit image
    B, B, A, A.  An odd-sized ellipse is symmetric, so its (dilate, erode) is a closing and idempotent: after the first
    launch of iterations 3 and 4 (4 passes, two whole iterations) the other image already holds the final bits.  Hence
    ksize 15, iterations 5 as well: reach 7 allows 64 / 7 = 9 of the 10 passes (158 rows, 6 * 158 * 64 B = 60672 B),
    so the launches are 9 + 1, the result is in A and B holds the state after a dilate."""
    h, w = 60, 200
    flows = _sparse_flows(torch_dev, 13, 2, h, w, 0.25)
    boxes = [[(0, 0, 150, 50), (40, 10, 197, 60)], [(0, 0, w, h)]]
    got = _check_both_entries(nsof_lib, ctx, oracle, flows, boxes, ksize=ksize, iterations=iterations)
    assert 0 < (got[1] != 0).sum() < got[1].size


@pytest.mark.gpu
def test_identity_pass_on_both_entries(nsof_lib, ctx, oracle, torch_dev):
    """iterations 0: one pass with the 1 x 1 element, on a 1 x 1 box and a 33 x 65 box."""
    h, w = 40, 70
    flows = _sparse_flows(torch_dev, 14, 2, h, w, 0.8)
    flows[0, 7, 5] = flows.new_tensor([3.0, 0.0])                  # the 1 x 1 box holds a set pixel
    boxes = [[(5, 7, 6, 8)], [(2, 4, 67, 37)]]
    got = _check_both_entries(nsof_lib, ctx, oracle, flows, boxes, iterations=0)
    assert got[0].sum() == 255 and got[0, 7, 5] == 255
    assert 0 < (got[1, 4:37, 2:67] != 0).sum() < 33 * 65
    mag = np.hypot(*np.moveaxis(flows[1].cpu().numpy().astype(np.float64), -1, 0))
    assert np.array_equal(got[1, 4:37, 2:67] != 0, mag[4:37, 2:67] > 1)


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(1080, 1920), (1920, 1080)])
def test_mask_sequence_whole_frame(nsof_lib, ctx, oracle, torch_dev, hw):
    from nsof import segment
    h, w = hw
    flows = _random_flows(torch_dev, 2, 2, h, w)
    got = segment.motion_mask_sequence_dev(flows, None, ctx=ctx)
    ctx.synchronize()
    got = got.cpu().numpy()
    assert np.array_equal(got, _per_box(nsof_lib, ctx, flows, None))
    assert np.array_equal(got[:1], _per_box_oracle(oracle, flows[:1].cpu().numpy(), None))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (37, 53), (121, 161), (8, 300)])
def test_pixel_accuracy_batch_equals_host(nsof_lib, ctx, torch_dev, shape):
    import torch
    from nsof import pipeline, segment
    h, w = shape
    n = 300
    rng = np.random.default_rng(h * 1000 + w)
    masks = np.where(rng.random((n, h, w)) < 0.4, np.uint8(255), np.uint8(0))
    gts = rng.integers(90, 166, (n, h, w, 3), dtype=np.uint8)      # gray values straddle 127
    gts[::7] = 255
    masks[::11] = 0
    big = torch.from_numpy(np.pad(gts, ((0, 0), (0, 3), (0, 0), (0, 0)))).to(torch_dev)   # strided frames
    d_gt = big[:, :h]
    torch.cuda.synchronize()
    got = segment.pixel_accuracy_batch_dev(torch.from_numpy(masks).to(torch_dev), d_gt, ctx=ctx)
    ctx.synchronize()
    got = got.cpu().numpy()
    for i in range(n):
        assert got[i] == pipeline.calculate_pixel_accuracy(masks[i], _gt_binary(gts[i])), i


def _run_both(nsof_lib, ctx, torch_dev, frames, gts, stack, cfg_kw, name, merge_flag):
    import torch
    from nsof import pipeline, segment
    masks = []

    def rec(f):
        out = segment.motion_mask(f, 1, ctx=ctx)
        masks.append(out.copy())
        return out

    cfg = nsof_lib.dataset_config(name, **cfg_kw)
    fl = lambda a, b, f, **kw: nsof_lib.calcOpticalFlowFarneback(a, b, f, **kw, ctx=ctx)  # noqa: E731
    rows, m_mem, m_orig = pipeline.run_segmentation(frames, gts, stack, cfg, merge_flag=merge_flag, flow_fn=fl,
                                                    mask_fn=rec)
    d = torch.from_numpy(np.stack(frames)).to(torch_dev)
    g = torch.from_numpy(np.stack(gts)).to(torch_dev)
    torch.cuda.synchronize()
    res = pipeline.segmentation_sequence_dev(d, g, stack, nsof_lib.dataset_config(name, **cfg_kw), merge_flag=merge_flag,
                                             ctx=ctx)
    mm, mo = res["mask_mem"].cpu().numpy(), res["mask_orig"].cpu().numpy()
    pm, po = res["pa_mem"].cpu().numpy(), res["pa_orig"].cpu().numpy()
    n_pairs = len(frames) - 2
    h, w = frames[0].shape[:2]
    assert len(rows) == n_pairs and mm.shape == (n_pairs, h, w)
    it = iter(masks)
    for k in range(n_pairs):
        want = np.zeros((h, w), np.uint8)                             # what run_segmentation pasted, in its order
        for x0, y0, x1, y1 in res["boxes"][k]:
            if x1 > x0 and y1 > y0:
                want[y0:y1, x0:x1] = next(it)
        assert np.array_equal(mm[k], want), (name, k, "mem")
        assert np.array_equal(mo[k], next(it)), (name, k, "orig")
        gt = _gt_binary(gts[k + 1])
        assert pm[k] == pipeline.calculate_pixel_accuracy(mm[k], gt) and rows[k][9] == f"{pm[k]:.4f}", (name, k)
        assert po[k] == pipeline.calculate_pixel_accuracy(mo[k], gt) and rows[k][8] == f"{po[k]:.4f}", (name, k)
    assert next(it, None) is None
    assert res["mean_mem"] == m_mem and res["mean_orig"] == m_orig
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("bug_compatible", [True, False])
def test_segmentation_sequence_dev_equals_harness_1080p(nsof_lib, ctx, torch_dev, bug_compatible):
    from nsof import workload as wl
    with np.load(os.path.join(GOLDEN, "gating_stacks.npz")) as z:
        stack = z["grasp"]
    h, w = wl.DATASET_FRAMES["grasp"][:2]
    frames = _synthetic_bgr(21, 6, h, w)
    gts = _synthetic_gt(22, 6, h, w)
    res = _run_both(nsof_lib, ctx, torch_dev, frames, gts, stack, dict(bug_compatible=bug_compatible), "grasp", False)
    assert res["boxes"] == res["rects"] and all(len(b) == 1 for b in res["boxes"])


def _load_gray3(path):
    pil = pytest.importorskip("PIL.Image")
    a = np.asarray(pil.open(path).convert("L"))
    return np.ascontiguousarray(np.repeat(a[..., None], 3, 2))    # cv2.imread of a one-channel JPEG


@pytest.mark.gpu
@pytest.mark.parametrize("name", DATASETS)
def test_segmentation_sequence_dev_equals_harness_real_frames(nsof_lib, ctx, torch_dev, name):
    pil = pytest.importorskip("PIL.Image")
    d = os.path.join(GOLDEN, "frames", name)
    files = sorted(os.listdir(d), key=lambda s: int(s.split(".")[0]))
    frames = [np.ascontiguousarray(np.asarray(pil.open(os.path.join(d, f)).convert("RGB"))[..., ::-1]) for f in files]
    gts = [_load_gray3(os.path.join(GOLDEN, "gtmask", name, f)) for f in files]
    assert gts[0].shape == frames[0].shape
    with np.load(os.path.join(GOLDEN, "gating_stacks.npz")) as z:
        stack = z[name]
    merges = (True, False) if nsof_lib.dataset_config(name).FLAG == 1 else (False,)
    for merge in merges:
        _run_both(nsof_lib, ctx, torch_dev, frames, gts, stack, {}, name, merge)


@pytest.mark.gpu
def test_segmentation_sequence_dev_small_memsize_overlaps(nsof_lib, ctx, torch_dev):
    stack = _json_stack("grasp", ("0", "1", "2", "3", "50"))
    hm, wm = stack.shape[:2]
    h, w = hm * 16, wm * 16
    frames = _synthetic_bgr(31, 6, h, w)
    gts = _synthetic_gt(32, 6, h, w)
    kw = dict(SMALL, FLAG=1, EXTEND_HEIGHT_UPPER=24, EXTEND_HEIGHT_LOWER=24, EXTEND_WIDTH_LEFT=24, EXTEND_WIDTH_RIGHT=24)
    for merge in (False, True):
        res = _run_both(nsof_lib, ctx, torch_dev, frames, gts, stack, kw, "grasp", merge)
        if not merge:
            overl = any(a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]
                        for bs in res["boxes"] for i, a in enumerate(bs) for b in bs[i + 1:])
            assert overl, res["boxes"]                          # extended rectangles overlap


@pytest.mark.gpu
def test_bad_inputs_raise_and_launch_nothing(nsof_lib, torch_dev):
    import torch
    from nsof import _lib, pipeline, segment
    from nsof.errors import NsofValueError
    c = nsof_lib.Context(0)
    try:
        c.prof_enable(_lib.K_SEGMENT, _lib.K_MORPH)
        fl = torch.zeros((3, 32, 40, 2), dtype=torch.float32, device=torch_dev)
        m = torch.zeros((3, 32, 40), dtype=torch.uint8, device=torch_dev)
        gt = torch.zeros((3, 32, 40, 3), dtype=torch.uint8, device=torch_dev)
        torch.cuda.synchronize()
        with pytest.raises(NsofValueError):
            segment.motion_mask_sequence_dev(fl.double(), ctx=c)
        with pytest.raises(NsofValueError):
            segment.motion_mask_sequence_dev(fl[:, :, :, :1], ctx=c)
        with pytest.raises(NsofValueError):
            segment.motion_mask_sequence_dev(fl.cpu(), ctx=c)
        with pytest.raises(NsofValueError):
            segment.motion_mask_sequence_dev(fl, [[], []], ctx=c)         # 2 box lists for 3 pairs
        with pytest.raises(NsofValueError):
            segment.motion_mask_sequence_dev(fl, out=m[:2], ctx=c)
        with pytest.raises(NsofValueError):
            segment.pixel_accuracy_batch_dev(m.float(), gt, ctx=c)
        with pytest.raises(NsofValueError):
            segment.pixel_accuracy_batch_dev(m, gt[:, :, :39], ctx=c)
        with pytest.raises(NsofValueError):
            segment.pixel_accuracy_batch_dev(m, gt, out=torch.zeros(3, device=torch_dev), ctx=c)
        with pytest.raises(NsofValueError):
            pipeline.segmentation_sequence_dev(gt, gt[:2], np.zeros((2, 2, 9)), nsof_lib.dataset_config("grasp"), ctx=c)

        def seq(n, counts, boxes, ksize=10, iterations=5):
            cn = None if counts is None else np.ascontiguousarray(counts, np.int32)
            bx = None if boxes is None else np.ascontiguousarray(boxes, np.int32).reshape(-1, 4)
            return c._lib.nsof_motion_mask_sequence_dev(c.ptr, n, fl.data_ptr(), 40, 32,
                                                        None if cn is None else cn.ctypes.data,
                                                        None if bx is None else bx.ctypes.data, 1.0, ksize, iterations,
                                                        m.data_ptr())
        assert seq(3, [1, 0, 0], [(0, 0, 41, 32)]) == _lib.NSOF_EINVAL         # leaves the frame
        assert seq(3, [0, 1, 0], [(-1, 0, 10, 10)]) == _lib.NSOF_EINVAL
        assert seq(3, [0, 0, 1], [(0, 30, 10, 33)]) == _lib.NSOF_EINVAL
        assert seq(0, None, None) == _lib.NSOF_ESHAPE
        assert seq(65536, None, None) == _lib.NSOF_EUNSUPPORTED
        assert seq(3, None, None, ksize=0) == _lib.NSOF_EUNSUPPORTED
        assert seq(3, None, None, ksize=33) == _lib.NSOF_EUNSUPPORTED
        assert seq(3, None, None, iterations=-1) == _lib.NSOF_EINVAL
        assert seq(3, None, None, iterations=17) == _lib.NSOF_EINVAL
        d = torch.zeros((3,), dtype=torch.float64, device=torch_dev)
        torch.cuda.synchronize()
        assert c._lib.nsof_pixel_accuracy_u8_batch_dev(c.ptr, 0, m.data_ptr(), gt.data_ptr(), 120, 3840, 40, 32,
                                                       d.data_ptr()) == _lib.NSOF_ESHAPE
        assert c._lib.nsof_pixel_accuracy_u8_batch_dev(c.ptr, 3, m.data_ptr(), gt.data_ptr(), 119, 3840, 40, 32,
                                                       d.data_ptr()) == _lib.NSOF_EINVAL
        assert c.prof_collect(_lib.K_SEGMENT)[1] == 0 and c.prof_collect(_lib.K_MORPH)[1] == 0
    finally:
        c.close()
