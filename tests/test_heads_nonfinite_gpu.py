"""GPU: the heads that consume a flow on the device -- the colour coding (csrc/flowviz_kernels.hip), the prediction warp
(csrc/warp_kernels.hip: remap, fused warp, sequence warp) and the motion mask (mag_pack_rows of csrc/segment_kernels.hip in both
of its kernels) -- on flows that are partly NaN, infinite, beyond float32's square range, subnormal or -0.0: the hand-made
fields of tests/heads_nonfinite_cases.py, and a float-frame Farneback flow that is NaN on most of its pixels.

Every comparison is exact (``np.array_equal`` on uint8 output, bit equality on the float32 divisors) against a CPU
reference: ``cr_flow_to_image_nonfinite`` (tests/test_flowviz_cpu.py), ``oracle.flow_map`` + ``oracle.remap_linear``,
``oracle.motion_mask``.  What those references make of the same fields is pinned without a device in
tests/test_heads_nonfinite_cpu.py."""
import itertools

import numpy as np
import pytest

import heads_nonfinite_cases as K
from test_flowviz_cpu import cr_flow_to_image_nonfinite
from test_nonfinite_cpu import REMAP_BAD

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- colour coding
def _upload(torch_dev, flows, path):
    """Host flows [..][h][w][2] on the device, as the load path asks: "float4" a contiguous tensor (16-byte aligned
    rows), "scalar" a view at an odd x offset of a canvas whose every other value is +inf (rows 8 bytes off a 16-byte
    boundary; a kernel that read past the crop would get an infinite divisor)."""
    import torch
    flows = np.ascontiguousarray(flows, np.float32)
    if path == "float4":
        t = torch.from_numpy(flows).to(torch_dev)
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        return t
    h, w = flows.shape[-3], flows.shape[-2]
    cw = w + 8 + (w % 2)                                   # even: every row is as far off the boundary as the first
    canvas = np.full(flows.shape[:-3] + (h + 3, cw, 2), np.inf, np.float32)
    canvas[..., 2:2 + h, 3:3 + w, :] = flows
    t = torch.from_numpy(canvas).to(torch_dev)[..., 2:2 + h, 3:3 + w, :]
    assert t.data_ptr() % 16 == 8 and (h * w == 1 or not t.is_contiguous())
    return t


def _colour(ctx, torch_dev, flows, path, **kw):
    """flow_to_image_dev on the uploaded flows -> (host images, host divisors)."""
    import torch
    from nsof import flowviz
    t = _upload(torch_dev, flows, path)
    n = 1 if t.dim() == 3 else int(t.shape[0])
    norms = torch.full((n,), -1.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    out = flowviz.flow_to_image_dev(t, norms=norms, ctx=ctx, **kw)
    ctx.synchronize()
    return out.cpu().numpy(), norms.cpu().numpy()


def _colour_variants():
    for sign, clip, bgr in itertools.product((1, -1), (None, 2.5), (False, True)):
        yield dict(sign=sign, clip_flow=clip, convert_to_bgr=bgr)


def _colour_want(flow, sign=1, **kw):
    return cr_flow_to_image_nonfinite(-flow if sign < 0 else flow, **kw)


@pytest.mark.parametrize("path", ["float4", "scalar"])
def test_colour_nan_only_field(nsof_lib, ctx, torch_dev, path):
    """NaN pixels are black and stay out of the divisor, which is finite: everything else keeps its ordinary colour."""
    flow = K.colour_fields()["nan"]
    for kw in _colour_variants():
        want, d = _colour_want(flow, **kw)
        got, norms = _colour(ctx, torch_dev, flow, path, **kw)
        assert np.isfinite(d) and _bits(norms)[0] == _bits(d), (kw, norms, d)
        assert np.array_equal(got, want), (kw, int((got != want).any(-1).sum()))
        assert len(np.unique(got.reshape(-1, 3), axis=0)) > 50, kw


@pytest.mark.parametrize("path", ["float4", "scalar"])
def test_colour_infinite_divisor_field(nsof_lib, ctx, torch_dev, path):
    """Infinite and overflowing magnitudes: the divisor is +inf (finite again under the clip)."""
    flow = K.colour_fields()["inf"]
    for kw in _colour_variants():
        want, d = _colour_want(flow, **kw)
        got, norms = _colour(ctx, torch_dev, flow, path, **kw)
        assert np.isposinf(d) == (kw["clip_flow"] is None) and _bits(norms)[0] == _bits(d), (kw, norms, d)
        assert np.array_equal(got, want), (kw, int((got != want).any(-1).sum()))


@pytest.mark.parametrize("path", ["float4", "scalar"])
@pytest.mark.parametrize("max_flow", [0.5, 3.0])
def test_colour_infinite_flow_under_max_flow(nsof_lib, ctx, torch_dev, path, max_flow):
    """A finite divisor from max_flow: an infinite component is a pixel outside the unit circle, not a black one."""
    fields = K.colour_fields()
    for name in ("inf", "nan"):
        flow = fields[name]
        for kw in _colour_variants():
            want, d = _colour_want(flow, max_flow=max_flow, **kw)
            got, norms = _colour(ctx, torch_dev, flow, path, max_flow=max_flow, **kw)
            assert _bits(norms)[0] == _bits(d) == _bits(np.float32(max_flow + 1e-5)), (name, kw)
            assert np.array_equal(got, want), (name, kw, int((got != want).any(-1).sum()))
    inf_px = np.isinf(fields["inf"]).any(-1) & ~np.isnan(fields["inf"]).any(-1)
    got, _ = _colour(ctx, torch_dev, fields["inf"], path, max_flow=max_flow)
    assert (got[inf_px] != 0).any(-1).all()


@pytest.mark.parametrize("path", ["float4", "scalar"])
def test_colour_batch_keeps_each_items_divisor(nsof_lib, ctx, torch_dev, path):
    """The three fields in one call: one item's +inf stays in its own slot, and a finite flow coded afterwards on the
    same context (the slots are the context's workspace) is what it is on its own."""
    fields = K.colour_fields()
    stack = np.stack([fields["nan"], fields["inf"], fields["finite"]])
    for kw in (dict(), dict(sign=-1, convert_to_bgr=True), dict(clip_flow=2.5)):
        got, norms = _colour(ctx, torch_dev, stack, path, **kw)
        want = [_colour_want(f, **kw) for f in stack]
        assert np.array_equal(_bits(norms), _bits([d for _, d in want])), (kw, norms)
        for k in range(3):
            assert np.array_equal(got[k], want[k][0]), (kw, k)
        if "clip_flow" not in kw:
            assert np.isfinite(norms[0]) and np.isposinf(norms[1]) and np.isfinite(norms[2])
        after, d_after = _colour(ctx, torch_dev, fields["finite"], path, **kw)
        assert _bits(d_after)[0] == _bits(want[2][1]) and np.array_equal(after, want[2][0]), kw
    # the order of the items does not matter either
    got, norms = _colour(ctx, torch_dev, stack[::-1], path)
    assert np.array_equal(_bits(norms), _bits([_colour_want(f)[1] for f in stack[::-1]]))


@pytest.mark.parametrize("path", ["float4", "scalar"])
@pytest.mark.parametrize("shape", K.COLOUR_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_colour_shapes_with_nan_in_last_row_and_column(nsof_lib, ctx, torch_dev, shape, path):
    """Sizes on the edges of the 256-px by 16-row workgroup and of the 4-px lane."""
    flow = K.shape_field(*shape)
    for kw in (dict(), dict(sign=-1, clip_flow=2.5, convert_to_bgr=True), dict(max_flow=3.0)):
        want, d = _colour_want(flow, **kw)
        got, norms = _colour(ctx, torch_dev, flow, path, **kw)
        assert _bits(norms)[0] == _bits(d), (kw, norms, d)
        assert np.array_equal(got, want), (kw, int((got != want).any(-1).sum()))


# ---------------------------------------------------------------------------------------------------- remap
@pytest.mark.parametrize("border", [0, 1])
def test_remap_special_maps(nsof_lib, oracle, ctx, border):
    """k_remap_u8<1|3, false>: NaN, +-inf, +-1e10 and the first values past the int range, in x, in y and in both, on
    the 9x13 source of tests/test_nonfinite_cpu.py; the same maps, and taps around the right and left edge, on
    3-channel sources narrower than the 8-byte two-tap load."""
    rng = np.random.default_rng(5)
    bad = REMAP_BAD + [2.0 ** 26 - 4]
    cases = [((9, 13), 1), ((9, 13), 3)] + [(s, 3) for s in K.REMAP_SOURCES_3CH] + [(s, 1) for s in K.REMAP_SOURCES_3CH]
    for (sh, sw), cn in cases:
        src = rng.integers(1, 255, (sh, sw) if cn == 1 else (sh, sw, cn), dtype=np.uint8)
        for default in ((2.25, 3.5), (0.25, 0.5)):
            mx, my = K.remap_maps(sw, sh, bad, default)
            got = nsof_lib.remap(src, mx, my, nsof_lib.INTER_LINEAR, borderMode=border, borderValue=7, ctx=ctx)
            want = oracle.remap_linear(src, mx, my, border, 7)
            assert np.array_equal(got, want), (sh, sw, cn, default, np.argwhere(got != want)[:4].tolist())


# ---------------------------------------------------------------------------------------------------- fused warp
def _warp_want(oracle, frame, flow, rect, sign, border):
    x0, y0, x1, y1 = rect
    want = frame.copy()
    mx, my = oracle.flow_map(flow, rect, sign)
    want[y0:y1, x0:x1] = oracle.remap_linear(frame, mx, my, border)
    return want


@pytest.mark.parametrize("cn", [1, 3])
def test_fused_warp_special_flows(nsof_lib, oracle, ctx, torch_dev, cn):
    """k_remap_u8<1|3, true>: the map is formed in double from the flow inside the kernel."""
    import torch
    rng = np.random.default_rng(6 + cn)
    h, w = K.H, K.W
    frame = rng.integers(1, 256, (h, w) if cn == 1 else (h, w, cn), dtype=np.uint8)
    flow = K.warp_flow(301)
    d_frame, d_flow = torch.from_numpy(frame).to(torch_dev), torch.from_numpy(flow).to(torch_dev)
    for rect, sign, border in itertools.product(K.WARP_RECTS, (1, -1), (0, 1)):
        want = _warp_want(oracle, frame, flow, rect, sign, border)
        got = nsof_lib.predict_region(frame, flow, rect, sign=sign, borderMode=border, ctx=ctx)
        assert np.array_equal(got, want), ("host", rect, sign, border, np.argwhere(got != want)[:4].tolist())
        d_out = d_frame.clone()
        torch.cuda.synchronize()
        nsof_lib.predict_region_dev(d_frame, d_flow, d_out, h, w, rect, channels=cn, sign=sign, borderMode=border, ctx=ctx)
        ctx.synchronize()
        got = d_out.cpu().numpy()
        assert np.array_equal(got, want), ("dev", rect, sign, border, np.argwhere(got != want)[:4].tolist())
    # the reference's float64 canvas, holding the same inf and NaN
    f64 = flow.astype(np.float64)
    assert np.isinf(f64).any() and np.isnan(f64).any()
    for rect, border in itertools.product(K.WARP_RECTS, (0, 1)):
        got = nsof_lib.predict_region(frame, f64, rect, sign=-1, borderMode=border, ctx=ctx)
        assert np.array_equal(got, _warp_want(oracle, frame, flow, rect, -1, border)), (rect, border)


# ---------------------------------------------------------------------------------------------------- sequence warp
def _sequence_case(torch_dev):
    import torch
    rng = np.random.default_rng(8)
    frames = rng.integers(1, 256, (3, K.H, K.W, 3), dtype=np.uint8)
    flows = np.stack([K.warp_flow(302), K.warp_flow(303)])
    return frames, flows, torch.from_numpy(frames).to(torch_dev), torch.from_numpy(flows).to(torch_dev)


def _full_warp(oracle, frame, flow, sign, border):
    mx, my = oracle.flow_map(flow, (0, 0, K.W, K.H), sign)
    return oracle.remap_linear(frame, mx, my, border)


@pytest.mark.parametrize("border", [0, 1])
def test_sequence_warp_without_a_table(nsof_lib, oracle, ctx, torch_dev, border):
    """k_predict_seq_u8<false>: every pair's whole frame."""
    frames, flows, d_frames, d_flows = _sequence_case(torch_dev)
    for sign in (-1, 1):
        got = nsof_lib.predict_sequence_dev(d_frames, d_flows, border_mode=border, sign=sign, ctx=ctx)
        ctx.synchronize()
        got = got.cpu().numpy()
        for k in range(2):
            want = _full_warp(oracle, frames[k + 1], flows[k], sign, border)
            assert np.array_equal(got[k], want), (sign, k, np.argwhere(got[k] != want)[:4].tolist())


@pytest.mark.parametrize("border", [0, 1])
def test_sequence_warp_with_a_table(nsof_lib, oracle, ctx, torch_dev, border):
    """k_predict_seq_u8<true>: the warp inside the table row's region (two overlapping rectangles, none, one on the
    frame's edge; as they are or merged with a padding of 5), the frame itself outside."""
    import torch
    frames, flows, d_frames, d_flows = _sequence_case(torch_dev)
    counts = torch.tensor(K.SEQ_COUNTS, dtype=torch.int32, device=torch_dev)
    rects = torch.tensor(K.SEQ_RECTS, dtype=torch.int32, device=torch_dev)
    assert tuple(rects.shape) == (3, 3, 4)
    torch.cuda.synchronize()
    full = [_full_warp(oracle, frames[k + 1], flows[k], -1, border) for k in range(2)]
    for gate_frame, merge in itertools.product((0, 1), (None, 5)):
        got = nsof_lib.predict_sequence_dev(d_frames, d_flows, counts=counts, rects=rects, gate_frame=gate_frame,
                                            merge_padding=merge, border_mode=border, ctx=ctx)
        ctx.synchronize()
        got = got.cpu().numpy()
        for k in range(2):
            g = k + gate_frame
            region = K.region_of(K.SEQ_RECTS[g][:K.SEQ_COUNTS[g]], K.H, K.W, merge)
            assert region.any() == (K.SEQ_COUNTS[g] > 0) and not region.all()
            want = np.where(region[..., None], full[k], frames[k + 1])
            assert np.array_equal(got[k][~region], frames[k + 1][~region]), (gate_frame, merge, k)
            assert np.array_equal(got[k], want), (gate_frame, merge, k, np.argwhere(got[k] != want)[:4].tolist())


# ---------------------------------------------------------------------------------------------------- motion mask
@pytest.mark.parametrize("chain", K.MASK_CHAINS, ids=lambda c: f"iters{c[0]}_k{c[1]}")
def test_motion_mask_special_flows(nsof_lib, oracle, ctx, torch_dev, chain):
    """k_mag_pack (host and device entries) and k_mag_pack_jobs (the sequence entry, two boxes per pair of which one
    touches the frame's edge): the float64 magnitude against the threshold, NaN never above it."""
    import torch
    from nsof import segment
    iters, ksize = chain
    h, w = K.MASK_H, K.MASK_W
    cases = K.mask_flows()
    flows = np.stack([f for f, _ in cases])
    d_flows = torch.from_numpy(flows).to(torch_dev)
    d_mask = torch.empty((h, w), dtype=torch.uint8, device=torch_dev)
    torch.cuda.synchronize()
    for k, (flow, marks) in enumerate(cases):
        want = oracle.motion_mask(flow, 1.0, ksize, iters)
        assert set(np.unique(want).tolist()) == {0, 255}
        if iters == 0:                                     # the oracle alone first: the threshold is the float64 one
            nan = np.isnan(flow).any(-1)
            assert not want[nan].any() and want[np.isinf(flow).any(-1) & ~nan].all()
            assert want[(np.abs(flow) == np.float32(3e38)).any(-1) & ~nan].all()
            assert np.array_equal(want, K.float64_mask(flow))
        got = segment.motion_mask(flow, 1, ksize, iters, ctx=ctx)
        assert np.array_equal(got, want), ("host", k, np.argwhere(got != want)[:4].tolist())
        got64 = segment.motion_mask(flow.astype(np.float64), 1, ksize, iters, ctx=ctx)
        assert np.array_equal(got64, want), ("host float64 canvas", k)
        segment.motion_mask_dev(d_flows[k], d_mask, h, w, 1, ksize, iters, ctx=ctx)
        ctx.synchronize()
        got = d_mask.cpu().numpy()
        assert np.array_equal(got, want), ("dev", k, np.argwhere(got != want)[:4].tolist())
    for boxes in (None, [list(b) for b in K.MASK_BOXES]):
        got = segment.motion_mask_sequence_dev(d_flows, boxes, seg_th=1, ksize=ksize, iterations=iters, ctx=ctx)
        ctx.synchronize()
        got = got.cpu().numpy()
        for k in range(2):
            want = np.zeros((h, w), np.uint8)
            for x0, y0, x1, y1 in (boxes[k] if boxes else [(0, 0, w, h)]):
                want[y0:y1, x0:x1] = oracle.motion_mask(np.ascontiguousarray(flows[k, y0:y1, x0:x1]), 1.0, ksize, iters)
            assert np.array_equal(got[k], want), ("sequence", boxes is not None, k, np.argwhere(got[k] != want)[:4].tolist())


def test_motion_mask_threshold_above_float32_range(nsof_lib, oracle, ctx, torch_dev):
    """seg_th = 1e39: (3e38, 3e38) has the float64 magnitude 4.2e38, below it; a float32 magnitude would be +inf."""
    import torch
    from nsof import segment
    h, w = K.MASK_H, K.MASK_W
    flows = np.stack([f for f, _ in K.mask_flows()])
    d_flows = torch.from_numpy(flows).to(torch_dev)
    d_mask = torch.empty((h, w), dtype=torch.uint8, device=torch_dev)
    torch.cuda.synchronize()
    seq = segment.motion_mask_sequence_dev(d_flows, None, seg_th=1e39, ksize=10, iterations=0, ctx=ctx)
    ctx.synchronize()
    for k in range(2):
        want = oracle.motion_mask(flows[k], 1e39, 10, 0)
        inf = np.isinf(flows[k]).any(-1) & ~np.isnan(flows[k]).any(-1)
        assert np.array_equal(want != 0, inf) and inf.any()
        assert np.array_equal(segment.motion_mask(flows[k], 1e39, 10, 0, ctx=ctx), want), k
        segment.motion_mask_dev(d_flows[k], d_mask, h, w, 1e39, 10, 0, ctx=ctx)
        ctx.synchronize()
        assert np.array_equal(d_mask.cpu().numpy(), want), k
        assert np.array_equal(seq[k].cpu().numpy(), want), k


# ---------------------------------------------------------------------------------------------------- end to end
def test_heads_on_a_partly_nan_farneback_flow(nsof_lib, oracle, ctx, torch_dev):
    """The way these values really arrive: float frames scaled to 4e20 make the Farneback flow NaN on most pixels.  The
    device flow is the oracle's on the bits (so a failure below is a head's, not the flow's); the heads then run on
    that device flow."""
    import torch
    from nsof import flowviz, segment
    prev, nxt, ref = K.farneback_nan_case(oracle)
    nan = np.isnan(ref).any(-1)
    assert nan.mean() >= 0.20 and np.isfinite(ref).all(-1).mean() >= 0.20, (nan.mean(), np.isfinite(ref).all(-1).mean())
    flow = nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, *K.FARNEBACK_ARGS, ctx=ctx)
    assert flow.dtype == np.float32 and flow.shape == ref.shape
    assert np.array_equal(np.isnan(flow), np.isnan(ref))
    assert np.array_equal(_bits(flow)[~np.isnan(ref)], _bits(ref)[~np.isnan(ref)])
    h, w = flow.shape[:2]
    d_flow = torch.from_numpy(flow).to(torch_dev)
    # colour coding
    norms = torch.full((1,), -1.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    for kw in (dict(), dict(sign=-1, convert_to_bgr=True), dict(clip_flow=2.5), dict(max_flow=3.0)):
        want, d = _colour_want(ref, **kw)
        got = flowviz.flow_to_image_dev(d_flow, norms=norms, ctx=ctx, **kw)
        ctx.synchronize()
        got = got.cpu().numpy()
        assert _bits(norms.cpu().numpy())[0] == _bits(d), (kw, d)
        assert np.array_equal(got, want), (kw, int((got != want).any(-1).sum()))
        assert np.array_equal((got == 0).all(-1), nan), kw
    # prediction warp, full frame
    frame = np.random.default_rng(9).integers(1, 256, (h, w, 3), dtype=np.uint8)
    d_frame = torch.from_numpy(frame).to(torch_dev)
    for border in (0, 1):
        want = _warp_want(oracle, frame, ref, (0, 0, w, h), -1, border)
        got = nsof_lib.predict_region(frame, flow, (0, 0, w, h), sign=-1, borderMode=border, ctx=ctx)
        assert np.array_equal(got, want), ("host", border)
        d_out = d_frame.clone()
        torch.cuda.synchronize()
        nsof_lib.predict_region_dev(d_frame, d_flow, d_out, h, w, (0, 0, w, h), sign=-1, borderMode=border, ctx=ctx)
        ctx.synchronize()
        assert np.array_equal(d_out.cpu().numpy(), want), ("dev", border)
        seq = nsof_lib.predict_sequence_dev(torch.stack([d_frame, d_frame]), d_flow[None], border_mode=border, ctx=ctx)
        ctx.synchronize()
        assert np.array_equal(seq[0].cpu().numpy(), want), ("sequence", border)
    # motion mask
    d_mask = torch.empty((h, w), dtype=torch.uint8, device=torch_dev)
    torch.cuda.synchronize()
    for iters, ksize in K.MASK_CHAINS:
        want = oracle.motion_mask(ref, 1.0, ksize, iters)
        assert set(np.unique(want).tolist()) == {0, 255}
        assert np.array_equal(segment.motion_mask(flow, 1, ksize, iters, ctx=ctx), want), (iters, ksize)
        segment.motion_mask_dev(d_flow, d_mask, h, w, 1, ksize, iters, ctx=ctx)
        ctx.synchronize()
        assert np.array_equal(d_mask.cpu().numpy(), want), (iters, ksize)
        seq = segment.motion_mask_sequence_dev(d_flow[None], None, seg_th=1, ksize=ksize, iterations=iters, ctx=ctx)
        ctx.synchronize()
        assert np.array_equal(seq[0].cpu().numpy(), want), (iters, ksize)
