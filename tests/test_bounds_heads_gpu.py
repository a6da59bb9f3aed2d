"""GPU: the head entries (gray, remap / warp, segmentation, colour coding, surfaces, SSIM, ROI table) write only their
outputs and read only their inputs -- the three assertions of tests/test_bounds_farneback_gpu.py: (a) the CPU reference
of the entry's present test, (b) bit-equal results under two poisons around the inputs, (c) a clean guard band around the
output (tests/guard_bands.py).

Entries that already had a check of the bytes next to their outputs when this file was written, and the test that makes it:

  nsof_accum_frames_f64*_dev, *_maps_dev, *_c2c_dev   sentinels behind every output: tests/test_frames_dev_gpu.py
                                                      (_guarded), test_frames_maps_gpu.py, test_frames_c2c_gpu.py
  nsof_accum_trials_dev and the plane checks          refused calls leave sentinel-filled outputs: test_accum_planes_gpu.py
  nsof_events_denoise_mark_dev / _compact_dev         poisoned outputs, test_events_denoise_gpu.py (_untouched)
  nsof_flow_ensemble_dev                              refusals leave the outputs untouched: test_flow_ensemble_gpu.py
  nsof_farneback_*_batch_desc_dev (float, 16-bit)     "nothing written outside the views": test_float_worklists_gpu.py,
                                                      test_int16_frames_gpu.py::test_device_pairs_on_crops
  nsof_flow_to_image_dev                              test_flowviz_gpu.py::test_strided_views_touch_only_the_crop (the
                                                      canvas around a strided crop; no band behind it, no input poison:
                                                      both added here)
  nsof_accum_surface_u8_dev / _f32_dev                row padding stays as it was: test_accum_gpu.py::
                                                      test_surface_u8_matches_host_map, test_float_input_gpu.py::
                                                      test_surface_f32_values (no band before or behind: added here)
  nsof_gray_u8_dev, nsof_predict_warp_u8_dev          the canvas around a crop: test_predict.py (no band, no poison: here)
"""

import numpy as np
import pytest

from guard_bands import banded_out, surrounded_in
from test_bounds_farneback_gpu import QNAN, _bits, _judge

pytestmark = pytest.mark.gpu

U8_POISONS = (np.uint8(0x00), np.uint8(0xFF))
F32_POISONS = (QNAN, np.float32(-1e30))


def _twice(ctx, what, poisons, run, want, tol=None):
    """run(poison) -> (out view, check): the entry called once per poison; then the three assertions."""
    runs = []
    for poison in poisons:
        out, check = run(poison)
        ctx.synchronize()
        runs.append((out.cpu().numpy(), check))
    _judge(what, runs, want, tol)
    return runs


# ---- nsof_gray_u8_dev: 4 pixels per thread, one packed dword where the destination is 4-byte aligned --------------------
@pytest.mark.parametrize("dst_offset", [0, 1, 2, 3])
@pytest.mark.parametrize("w", [1, 3, 4, 5, 1023, 1025])
def test_gray_u8(nsof_lib, ctx, torch_dev, w, dst_offset):
    import torch
    from nsof import gating
    for h in (1, 3):
        f = np.random.default_rng(w * 7 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        for bgr, code in ((0, "RGB2GRAY"), (1, "BGR2GRAY")):
            def run(poison):
                src = surrounded_in(torch, torch_dev, f, poison, pitch_extra=7, offset_elems=1, row_dims=2)
                out, check = banded_out(torch, torch_dev, (h, w), np.uint8, pitch_extra=5, offset_elems=dst_offset)
                ctx.check(ctx._lib.nsof_gray_u8_dev(ctx.ptr, src.data_ptr(), src.row_stride, w, h, bgr, out.data_ptr(),
                                                    out.row_stride))
                return out, check
            _twice(ctx, f"gray {(h, w)} {code} dst+{dst_offset}", U8_POISONS, run, gating.frame_to_gray(f, code))


# ---- nsof_remap_linear_u8_dev / nsof_predict_warp_u8_dev ----------------------------------------------------------------
@pytest.mark.parametrize("border", [0, 1], ids=["constant", "replicate"])
@pytest.mark.parametrize("cn", [1, 3])
def test_remap_linear(ctx, oracle, torch_dev, cn, border):
    """Source, both maps and the destination are crops with padded strides; the maps leave the source on every side."""
    import torch
    from test_predict import _maps
    rng = np.random.default_rng(cn * 10 + border)
    for (sh, sw), (dh, dw) in (((5, 3), (9, 70)), ((37, 53), (20, 131)), ((8, 8), (2, 1))):
        src = rng.integers(0, 256, (sh, sw) if cn == 1 else (sh, sw, cn), dtype=np.uint8)
        mx, my = _maps(rng, dh, dw, sw, sh)
        cval = 9 if border == 0 else 0
        want = oracle.remap_linear(src, mx, my, border, cval)

        def run(poison):
            pf = F32_POISONS[0] if poison == U8_POISONS[0] else F32_POISONS[1]
            d_src = surrounded_in(torch, torch_dev, src, poison, pitch_extra=5, offset_elems=1, row_dims=1 if cn == 1 else 2)
            d_mx = surrounded_in(torch, torch_dev, mx, pf, pitch_extra=3, offset_elems=1)
            d_my = surrounded_in(torch, torch_dev, my, pf, pitch_extra=2)
            out, check = banded_out(torch, torch_dev, want.shape, np.uint8, pitch_extra=6, offset_elems=1,
                                    row_dims=1 if cn == 1 else 2)
            ctx.check(ctx._lib.nsof_remap_linear_u8_dev(ctx.ptr, d_src.data_ptr(), d_src.row_stride, sw, sh, cn, d_mx.data_ptr(),
                                                        d_mx.row_stride // 4, d_my.data_ptr(), d_my.row_stride // 4, dw, dh,
                                                        border, cval, out.data_ptr(), out.row_stride))
            return out, check
        _twice(ctx, f"remap {(sh, sw)} -> {(dh, dw)} cn={cn} border={border}", U8_POISONS, run, want)


@pytest.mark.parametrize("border", [0, 1], ids=["constant", "replicate"])
@pytest.mark.parametrize("cn", [1, 3])
def test_predict_warp(ctx, oracle, torch_dev, cn, border):
    """The region of a frame-sized output (pre-filled with the frame, as the caller does) is overwritten; the rest of the
    frame, its row padding and the band stay."""
    import torch
    from test_predict import _want_region
    h, w = 40, 70
    rng = np.random.default_rng(cn + 2 * border)
    frame = rng.integers(0, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)
    flow = (rng.standard_normal((h, w, 2)) * 4).astype(np.float32)
    flow[:3] += 90.0     # footprints far outside the frame
    rd = 1 if cn == 1 else 2
    for rect in ((0, 0, w, h), (13, 7, 60, 33), (w - 1, h - 1, w, h), (0, 5, 64, 6)):
        x0, y0, x1, y1 = rect
        want = frame.copy()
        want[y0:y1, x0:x1] = _want_region(oracle, frame, flow, rect, -1, border)

        def run(poison):
            pf = F32_POISONS[0] if poison == U8_POISONS[0] else F32_POISONS[1]
            d_frame = surrounded_in(torch, torch_dev, frame, poison, pitch_extra=5, offset_elems=1, row_dims=rd)
            d_flow = surrounded_in(torch, torch_dev, flow, pf, pitch_extra=6, offset_elems=2, row_dims=2)
            out, check = banded_out(torch, torch_dev, frame.shape, np.uint8, pitch_extra=3, offset_elems=1, row_dims=rd)
            out.copy_(torch.from_numpy(frame).to(torch_dev))
            torch.cuda.synchronize()
            ctx.check(ctx._lib.nsof_predict_warp_u8_dev(ctx.ptr, d_frame.data_ptr(), d_frame.row_stride, w, h, cn,
                                                        d_flow.data_ptr(), d_flow.row_stride // 4, -1, x0, y0, x1, y1, border,
                                                        out.data_ptr(), out.row_stride))
            return out, check
        _twice(ctx, f"predict_warp {rect} cn={cn} border={border}", U8_POISONS, run, want)


@pytest.mark.parametrize("table", [False, True], ids=["whole_frame", "roi_table"])
def test_predict_sequence(ctx, oracle, torch_dev, table):
    """Two pairs in one launch: strided frames, dense flows and predictions.  With a table: pair k takes the rectangles of
    map k (overlapping boxes, a map without boxes), replicated borders; without: the whole frame, constant border 0."""
    import torch
    from test_predict import _want_region
    h, w, n_pairs = 23, 37, 2
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (n_pairs + 1, h, w, 3), dtype=np.uint8)
    flows = (rng.standard_normal((n_pairs, h, w, 2)) * 3).astype(np.float32)
    flows[0, :4] = 80.0
    lists = [[(3, 2, 20, 15), (10, 8, 37, 23)], [], [(0, 0, 5, 5)]]
    border = 1 if table else 0
    want = []
    for k in range(n_pairs):
        img = frames[k + 1].copy()
        for r in (lists[k] if table else [(0, 0, w, h)]):
            img[r[1]:r[3], r[0]:r[2]] = _want_region(oracle, frames[k + 1], flows[k], r, -1, border)
        want.append(img)
    want = np.stack(want)
    counts = torch.tensor([len(r) for r in lists], dtype=torch.int32, device=torch_dev)
    rects = torch.zeros((3, 2, 4), dtype=torch.int32)
    for k, rs in enumerate(lists):
        for i, r in enumerate(rs):
            rects[k, i] = torch.tensor(r)
    rects = rects.to(torch_dev)

    def run(poison):
        pf = F32_POISONS[0] if poison == U8_POISONS[0] else F32_POISONS[1]
        d_frames = surrounded_in(torch, torch_dev, frames, poison, pitch_extra=5, item_extra=11, offset_elems=1, row_dims=2)
        d_flows = surrounded_in(torch, torch_dev, flows, pf, row_dims=2)
        out, check = banded_out(torch, torch_dev, (n_pairs, h, w, 3), np.uint8, row_dims=2)
        ctx.check(ctx._lib.nsof_predict_sequence_u8_dev(
            ctx.ptr, n_pairs, d_frames.data_ptr(), d_frames.row_stride, d_frames.item_stride, w, h, d_flows.data_ptr(), -1,
            counts.data_ptr() if table else None, rects.data_ptr() if table else None, 3 if table else 0, 2 if table else 0, 0,
            -1, border, out.data_ptr()))
        return out, check
    _twice(ctx, f"predict_sequence table={table}", U8_POISONS, run, want)


# ---- the segmentation head ------------------------------------------------------------------------------------------------
SEG_SHAPES = [(h, w) for w in (1, 31, 33, 65) for h in (1, 9, 33)]   # the mask is packed 32 pixels to a word


def _seg_flow(seed, shape):
    """A flow whose magnitude lies on both sides of the threshold 1 in blobs (so that dilate / erode have work to do)."""
    h, w = shape
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((h, w, 2)) * 0.5).astype(np.float32)
    f[rng.random((h, w)) < 0.08] += np.float32(2.0)
    return f


@pytest.mark.parametrize("shape", SEG_SHAPES, ids=[f"{h}x{w}" for h, w in SEG_SHAPES])
def test_motion_mask(ctx, oracle, torch_dev, shape):
    import torch
    h, w = shape
    flow = _seg_flow(h * 100 + w, shape)
    for ksize, iters in ((10, 5), (3, 1)):
        want = oracle.motion_mask(flow, 1.0, ksize, iters)

        def run(poison):
            d_flow = surrounded_in(torch, torch_dev, flow, poison, pitch_extra=6, offset_elems=2, row_dims=2)
            out, check = banded_out(torch, torch_dev, (h, w), np.uint8, pitch_extra=3, offset_elems=1)
            ctx.check(ctx._lib.nsof_motion_mask_dev(ctx.ptr, d_flow.data_ptr(), d_flow.row_stride // 4, w, h, 1.0, ksize, iters,
                                                    out.data_ptr(), out.row_stride))
            return out, check
        _twice(ctx, f"motion_mask {shape} ksize={ksize} iterations={iters}", F32_POISONS, run, want)


@pytest.mark.parametrize("op", [0, 1], ids=["erode", "dilate"])
@pytest.mark.parametrize("shape", SEG_SHAPES, ids=[f"{h}x{w}" for h, w in SEG_SHAPES])
def test_morph_binary(ctx, oracle, torch_dev, shape, op):
    """0x00 around the source would erode, 0xFF would dilate, if a pixel outside the image took part."""
    import torch
    h, w = shape
    src = np.where(np.random.default_rng(h * 100 + w + op).random((h, w)) < (0.85 if op == 0 else 0.1), 255, 0).astype(np.uint8)
    for kw, kh, iters in ((10, 10, 1), (3, 5, 2)):
        elem = oracle.structuring_element(2, kw, kh)
        want = src
        for _ in range(iters):
            want = oracle.morph(op, want, elem)

        def run(poison):
            d_src = surrounded_in(torch, torch_dev, src, poison, pitch_extra=5, offset_elems=1)
            out, check = banded_out(torch, torch_dev, (h, w), np.uint8, pitch_extra=3, offset_elems=1)
            ctx.check(ctx._lib.nsof_morph_binary_u8_dev(ctx.ptr, op, d_src.data_ptr(), d_src.row_stride, w, h, elem.ctypes.data,
                                                        kw, kh, -1, -1, iters, out.data_ptr(), out.row_stride))
            return out, check
        _twice(ctx, f"morph op={op} {shape} elem {kw}x{kh} iterations={iters}", U8_POISONS, run, want)


@pytest.mark.parametrize("shape", [(9, 1), (9, 31), (33, 33), (33, 65)], ids=["9x1", "9x31", "33x33", "33x65"])
def test_motion_mask_sequence(ctx, oracle, torch_dev, shape):
    """Two pairs: one whole-frame box per pair (box_counts NULL), then box lists (overlapping, touching the edges, an empty
    list): every pixel of every canvas is written, 0 where no box covers it."""
    import torch
    h, w = shape
    flows = np.stack([_seg_flow(h * 100 + w + k, shape) for k in range(2)])
    lists = [[(0, 0, w, h)], [(0, 0, w, h)]]
    cases = [(None, lists)]
    if w >= 31:
        cases.append((True, [[(2, 1, 20, 8), (10, 3, w, h)], []]))
    for boxed, boxes in cases:
        want = np.zeros((2, h, w), np.uint8)
        for k in range(2):
            for x0, y0, x1, y1 in boxes[k]:
                want[k, y0:y1, x0:x1] = oracle.motion_mask(np.ascontiguousarray(flows[k, y0:y1, x0:x1]), 1.0, 10, 5)
        counts = np.array([len(b) for b in boxes], np.int32)
        tab = np.array([r for b in boxes for r in b], np.int32).reshape(-1, 4)

        def run(poison):
            d_flows = surrounded_in(torch, torch_dev, flows, poison, row_dims=2)
            out, check = banded_out(torch, torch_dev, (2, h, w), np.uint8)
            ctx.check(ctx._lib.nsof_motion_mask_sequence_dev(ctx.ptr, 2, d_flows.data_ptr(), w, h,
                                                             counts.ctypes.data if boxed else None,
                                                             tab.ctypes.data if boxed else None, 1.0, 10, 5, out.data_ptr()))
            return out, check
        _twice(ctx, f"motion_mask_sequence {shape} boxes={bool(boxed)}", F32_POISONS, run, want)


# ---- nsof_flow_to_image_dev -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 2], ids=["rows16B", "rows8B"])
@pytest.mark.parametrize("shape", [(21, 37), (5, 64), (1, 1)], ids=["21x37", "5x64", "1x1"])
def test_flow_to_image(ctx, torch_dev, shape, offset):
    """Two items with padded rows and items on both sides, the divisors in a band of their own.  -1e30 around the flows
    would become an item's maximum."""
    import torch
    from test_flowviz_cpu import cr_flow_to_image
    h, w = shape
    rng = np.random.default_rng(h + w)
    flows = np.stack([(rng.standard_normal((h, w, 2)) * s).astype(np.float32) for s in (0.5, 7.0)])
    want = np.stack([cr_flow_to_image(flows[k], convert_to_bgr=True) for k in range(2)])
    want_norm = np.array([[np.max(np.sqrt(np.square(f[..., 0]) + np.square(f[..., 1]))) + np.float32(1e-5) for f in flows]],
                         np.float32)
    norm_runs = []

    def run(poison):
        d_flows = surrounded_in(torch, torch_dev, flows, poison, pitch_extra=4, item_extra=8, offset_elems=offset, row_dims=2)
        out, check = banded_out(torch, torch_dev, (2, h, w, 3), np.uint8, pitch_extra=5, item_extra=7, offset_elems=1, row_dims=2)
        norms, ncheck = banded_out(torch, torch_dev, (1, 2), np.float32)
        ctx.check(ctx._lib.nsof_flow_to_image_dev(ctx.ptr, 2, d_flows.data_ptr(), d_flows.row_stride // 4, d_flows.item_stride // 4,
                                                  w, h, 1, -1.0, -1.0, 1, out.data_ptr(), out.row_stride, out.item_stride,
                                                  norms.data_ptr()))
        ctx.synchronize()
        norm_runs.append((norms.cpu().numpy(), ncheck))
        return out, check
    _twice(ctx, f"flow_to_image {shape} offset {offset}", F32_POISONS, run, want)
    _judge(f"flow_to_image norms {shape}", norm_runs, want_norm)


# ---- nsof_accum_surface_u8_dev / _f32_dev ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["state", "current"])
def test_accum_surfaces(nsof_lib, ctx, oracle, torch_dev, mode):
    """The surfaces of an accumulator after a short run, into padded rows one element past an aligned address.  The input is
    the accumulator's own state, so there is nothing to poison: the two runs are two calls.  The oracle's values outside
    its device band (oracle.accum_surface_*: the pixels whose value it cannot pin)."""
    import torch
    from nsof import synth
    from nsof.accumulator import Accumulator, slice_index_array
    H, W = 45, 67
    x, y, pol, t = synth.make_events(9, W, H, 3000, 40_000, box=(12, 9))
    acc = Accumulator(H, W, 1, "split", -6.0, 0.0, ctx=ctx)
    try:
        acc.step(x, y, pol, t, slice_index_array(t, 1000), snap_every=0)
        wst = acc.w(0)
        m = {"current": 0, "state": 1}[mode]
        for dtype, entry, ref in ((np.uint8, ctx._lib.nsof_accum_surface_u8_dev, oracle.accum_surface_u8),
                                  (np.float32, ctx._lib.nsof_accum_surface_f32_dev, oracle.accum_surface_f32)):
            want, band = ref(wst, mode)
            assert not band.all()
            runs = []
            for _ in range(2):
                out, check = banded_out(torch, torch_dev, (H, W), dtype, pitch_extra=3, offset_elems=1)
                ctx.check(entry(acc._p, 0, m, out.data_ptr(), out.row_stride))
                ctx.synchronize()
                got = out.cpu().numpy()
                assert np.array_equal(_bits(got)[~band], _bits(want)[~band]), (mode, dtype)
                runs.append((got, check))
            _judge(f"accum surface {mode} {np.dtype(dtype).name}", runs, None)
    finally:
        acc.close()


# ---- nsof_ssim_u8_batch_dev -------------------------------------------------------------------------------------------------
def test_ssim_batch(ctx, oracle, torch_dev):
    """Three pairs of one interleaved channel, padded rows and items, the three doubles in a band.  The score is held to
    the oracle within 1e-13, the bound of tests/test_predict.py (the window sums are exact integers on both sides; the
    final mean is summed in another order); assertions (b) and (c) are exact."""
    import torch
    n, h, w = 3, 11, 37
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-20, 21, a.shape), 0, 255).astype(np.uint8)
    want = np.array([[oracle.ssim_u8(a[i, :, :, 2], b[i, :, :, 2], 255.0) for i in range(n)]])
    runs = []
    for poison in U8_POISONS:
        da = surrounded_in(torch, torch_dev, a, poison, pitch_extra=5, item_extra=9, offset_elems=1, row_dims=2)
        db = surrounded_in(torch, torch_dev, b, poison, pitch_extra=2, item_extra=4, row_dims=2)
        out, check = banded_out(torch, torch_dev, (1, n), np.float64)
        ctx.check(ctx._lib.nsof_ssim_u8_batch_dev(ctx.ptr, n, da.data_ptr() + 2, da.row_stride, da.item_stride, 3, db.data_ptr() + 2,
                                                  db.row_stride, db.item_stride, 3, w, h, 255.0, out.data_ptr()))
        ctx.synchronize()
        got = out.cpu().numpy()
        assert np.abs(got - want).max() < 1e-13, (got, want)
        runs.append((got, check))
    _judge("ssim batch", runs, None)


# ---- nsof_roi_from_surface_dev -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(5, 5), (65, 3)], ids=["5x5_one_wave", "65x3_union_find"])
def test_roi_from_surface(ctx, torch_dev, rows, cols):
    """Three maps with padding between them; more components than max_rects = 2: the counts are the true numbers, the
    first two rectangles are stored and the rest of the table's rows for that map are beyond what the entry owns only in
    the sense that it may leave them: they are compared between the two runs, not with the reference."""
    import torch
    from nsof import gating
    ms, max_rects, n = 7, 2, 3
    h, w = rows * ms + 3, cols * ms + 5
    rng = np.random.default_rng(rows)
    on = rng.random((n, rows, cols)) < 0.4
    on[0] = (np.add.outer(np.arange(rows), np.arange(cols)) % 2) == 0     # a checkerboard: many components (4-connectivity)
    on[2] = False
    cur = np.where(on, 1e-5, 1e-9)
    cfg = gating.GatingConfig(MEMSIZE=ms, THRES=200, FLAG=1, CONNECT=4, EXTEND_HEIGHT_UPPER=2, EXTEND_HEIGHT_LOWER=3,
                              EXTEND_WIDTH_LEFT=1, EXTEND_WIDTH_RIGHT=4)
    want = [gating.roi_from_surface(cur[k], (h, w), cfg) for k in range(n)]
    assert len(want[0]) > max_rects and not want[2]
    want_counts = np.array([[len(v) for v in want]], np.int32)
    want_gray = np.stack([gating.current_to_gray(cur[k]) for k in range(n)])
    runs_c, runs_r, runs_g = [], [], []
    for poison in (np.float64(np.nan), np.float64(1e30)):
        d = surrounded_in(torch, torch_dev, cur, poison, item_extra=5)
        counts, c_check = banded_out(torch, torch_dev, (1, n), np.int32)
        rects, r_check = banded_out(torch, torch_dev, (n, max_rects, 4), np.int32)
        gray, g_check = banded_out(torch, torch_dev, (n, rows, cols), np.uint8)
        ctx.check(ctx._lib.nsof_roi_from_surface_dev(ctx.ptr, d.data_ptr(), n, d.item_stride // 8, rows, cols, w, h, cfg.MEMSIZE,
                                                     cfg.THRES, cfg.EXTEND_WIDTH_LEFT, cfg.EXTEND_WIDTH_RIGHT,
                                                     cfg.EXTEND_HEIGHT_UPPER, cfg.EXTEND_HEIGHT_LOWER, cfg.CONNECT, cfg.FLAG,
                                                     max_rects, counts.data_ptr(), rects.data_ptr(), gray.data_ptr()))
        ctx.synchronize()
        got_r = rects.cpu().numpy()
        for k in range(n):
            stored = min(len(want[k]), max_rects)
            assert [tuple(int(v) for v in r) for r in got_r[k, :stored]] == [tuple(r) for r in want[k][:stored]], (k, got_r[k])
        runs_c.append((counts.cpu().numpy(), c_check))
        runs_r.append((got_r, r_check))
        runs_g.append((gray.cpu().numpy(), g_check))
    _judge(f"roi counts {rows}x{cols}", runs_c, want_counts)
    _judge(f"roi rects {rows}x{cols}", runs_r, None)
    _judge(f"roi gray {rows}x{cols}", runs_g, want_gray)
