"""GPU: the frame-driven gating path in HBM -- Lanczos-3 compress of a frame stack (``frames.process_images_dev``), the
one-launch array run (``simulate_frames_dev``), their join (``pipeline.gating_stack_from_frames_dev``) feeding the
sequence experiments, and the refusals.  Everything is pinned bit for bit to the host chain
(``frames.process_images`` -> ``simulate_frames`` -> ``v_ds / resistances[1:]``)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = -777.25
GUARD = 16

# frame h x w, m, n  (-> out h // n x w // m)
COMPRESS_CASES = [
    (161, 161, 40, 40),   # 4x4, the uav case; a tie, so rows go first
    (80, 160, 16, 16),    # 5x10, a non-square tie
    (7, 300, 100, 7),     # 1x3: 41 taps over 7 rows (the mirror wraps three times), output length 1; columns first
    (50, 70, 7, 2),       # 25x10, columns first
    (33, 90, 45, 4),      # 8x2
    (45, 64, 8, 1),       # 45x8, scale 1 on rows
    (96, 128, 16, 16),    # 6x8
    # more than one tile on the axis that is not resized: k_resize_rows takes 256 columns per workgroup, k_resize_cols 64
    # rows, 32 taps per staging round (tests/test_frames_dev_cpu.py recomputes pass order, tile and tap counts of every case)
    (130, 600, 2, 2),     # 65x300, rows first: 3 column tiles (the last 88 wide), 2 row tiles (the last 1 row)
    (65, 257, 1, 1),      # 65x257, rows first: one element past the tile edge on both axes
    (64, 256, 1, 1),      # 64x256: exactly one full tile each
    (200, 520, 2, 1),     # 200x260, columns first over 4 row tiles (the last 8 rows) of the 8-bit source; rows: 2 tiles
    (150, 1030, 4, 2),    # 75x257, columns first over 3 row tiles; rows over the float64 intermediate, 2 tiles (the last 1)
    (130, 2600, 10, 1),   # 130x260, columns first: 60 taps = two staging rounds (32 + 28) in each of 3 row tiles
    (700, 66, 1, 10),     # 70x66, rows first with 60 taps; columns over the intermediate with 2 row tiles
]


def _resize_reversed(img, out_h, out_w):
    """``frames.imresize_lanczos3`` with every output's taps summed right to left."""
    from nsof import frames
    scales = (out_h / img.shape[0], out_w / img.shape[1])
    for ax in ((0, 1) if scales[0] <= scales[1] else (1, 0)):
        wts, ind = frames._contributions(img.shape[ax], (out_h, out_w)[ax], scales[ax])
        moved = np.moveaxis(img, ax, 0)
        out = np.zeros((wts.shape[0],) + moved.shape[1:], np.float64)
        for k in range(wts.shape[1] - 1, -1, -1):
            out += wts[:, k].reshape(-1, 1) * moved[ind[:, k]]
        img = np.moveaxis(out, 0, ax)
    return img


def _guarded(torch, dev, shape):
    """A contiguous float64 tensor of ``shape`` filled with a sentinel, GUARD sentinel elements behind it."""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=dev)
    return buf, buf[:n].view(shape)


@pytest.mark.parametrize("h,w,m,n", COMPRESS_CASES)
def test_compress_equals_the_mirror(nsof_lib, ctx, torch_dev, h, w, m, n):
    import torch
    from nsof import frames
    rng = np.random.default_rng(h * 1000 + w)
    oy, ox, hb, wb, pad = 3, 5, h + 6, w + 11, 13           # odd crop origin, row stride > width, padded frame stride
    a, b = (rng.integers(0, 256, (hb, wb), dtype=np.uint8) for _ in range(2))
    host = [a, b, a]
    ul, lr = (oy + 1, ox + 1), (oy + h, ox + w)
    ref = frames.process_images(host, m, n, ul, lr)
    assert ref.shape == (3, h // n, w // m)
    # bit equality checks the tap order: the other order gives other bits on these inputs
    rev = np.stack([_resize_reversed(frames.im2double(f[oy:oy + h, ox:ox + w]), h // n, w // m) for f in host])
    assert np.abs(rev - ref).max() < 1e-12 and not np.array_equal(rev, ref)

    base = torch.zeros((3, hb * wb + pad), dtype=torch.uint8, device=torch_dev)
    stack = base[:, :hb * wb].view(3, hb, wb)
    stack.copy_(torch.from_numpy(np.stack(host)))
    assert stack.stride() == (hb * wb + pad, wb, 1)
    buf, out = _guarded(torch, torch_dev, ref.shape)
    torch.cuda.synchronize(torch_dev)
    got = frames.process_images_dev(stack, m, n, ul, lr, out=out, ctx=ctx)
    ctx.synchronize()
    assert got is out
    res = buf.cpu().numpy()
    assert (res[-GUARD:] == SENTINEL).all()
    assert np.array_equal(res[:-GUARD].reshape(ref.shape), ref)
    assert np.array_equal(res[:ref[0].size], res[2 * ref[0].size:3 * ref[0].size])   # frame 2 is frame 0 again


GRIDS = [(1, 1), (4, 4), (6, 8), (13, 24)]
THRESHOLDS = [(0.7, 1.5), (2.0, 1.5)]
_array_refs = {}


def _array_case(nsof_lib, ctx, grid, th):
    """Five compressed frames of ``grid`` whose differences fall on both sides of the thresholds, and the host entry's
    result on them (computed once per case, shared, left unchanged)."""
    key = (grid, th)
    if key not in _array_refs:
        rng = np.random.default_rng(grid[0] * 100 + grid[1])
        base = rng.random(grid)
        step = rng.choice([0.0, 0.002, 0.01, 0.3], size=(5,) + grid) * rng.standard_normal((5,) + grid)
        imgs = np.clip(base + step, 0.0, 1.0)
        w, res = nsof_lib.simulate_frames(imgs, 5e-4, 50, th[0], th[1], ctx=ctx)
        for arr in (imgs, w, res):
            arr.setflags(write=False)
        _array_refs[key] = (imgs, w, res)
    return _array_refs[key]


@pytest.mark.parametrize("v_ds", [1.0, 0.5])
@pytest.mark.parametrize("th", THRESHOLDS)
@pytest.mark.parametrize("grid", GRIDS)
def test_array_run_equals_the_host_entry(nsof_lib, ctx, torch_dev, grid, th, v_ds):
    """Host and device entry run one kernel, so this pins the PLUMBING of the two against each other -- the copies, the
    layout of ``res`` and ``current``, ``v_ds``; the arithmetic itself is pinned by the recorded bits of
    ``tests/test_frames_bits_gpu.py``."""
    import torch
    imgs, w_ref, res_ref = _array_case(nsof_lib, ctx, grid, th)
    assert np.unique(res_ref).size > 2          # the array moves: not the initial resistance everywhere
    d = torch.from_numpy(imgs.copy()).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    w, res, cur = nsof_lib.simulate_frames_dev(d, 5e-4, 50, th[0], th[1], v_ds, ctx=ctx)
    ctx.synchronize()
    assert np.array_equal(w.cpu().numpy(), w_ref)
    assert np.array_equal(res.cpu().numpy(), res_ref)
    assert cur.shape == (4,) + grid and np.array_equal(cur.cpu().numpy(), v_ds / res_ref[1:])


def _moving_patch_frames():
    """Eight 96x128 BGR frames: a bright 28x36 patch moves 10 px right and 4 px down per frame over static texture."""
    rng = np.random.default_rng(11)
    texture = rng.integers(40, 120, (96, 128, 3), dtype=np.uint8)
    out = []
    for f in range(8):
        fr = texture.copy()
        fr[6 + 4 * f:6 + 4 * f + 28, 8 + 10 * f:8 + 10 * f + 36] = 250
        out.append(fr)
    return np.stack(out)


def test_join_feeds_the_sequence_experiments(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import frames, gating, pipeline
    cfg = gating.GatingConfig(MEMSIZE=16, THRES=245, OFFSET=0)
    bgr = _moving_patch_frames()
    # the host chain
    grays = [gating.frame_to_gray(f, "RGB2GRAY") for f in bgr]
    comp = frames.process_images(grays, 16, 16)
    _, res = nsof_lib.simulate_frames(comp, n_sub_steps=20, ctx=ctx)
    cur_host = 1.0 / res[1:]
    assert cur_host.shape == (7, 6, 8)
    gated = [int((gating.current_to_gray(c) >= cfg.THRES).sum()) for c in cur_host]
    print("gated cells per slice:", gated)
    assert any(0 < g < 48 for g in gated), gated      # precondition: the gate is neither shut nor wide open throughout

    d_bgr = torch.from_numpy(bgr).to(torch_dev)
    torch.cuda.synchronize(torch_dev)
    stack = pipeline.gating_stack_from_frames_dev(d_bgr, cfg, n_sub_steps=20, ctx=ctx)
    assert stack.dtype == torch.float64 and stack.is_cuda
    assert np.array_equal(stack.cpu().numpy(), cur_host)

    host_stack = np.moveaxis(cur_host, 0, 2)            # (rows, cols, T), the constructed3DMatrix layout
    p_dev = pipeline.prediction_sequence_dev(d_bgr, stack, cfg, ctx=ctx)
    p_host = pipeline.prediction_sequence_dev(d_bgr, host_stack, cfg, ctx=ctx)
    gt = torch.zeros_like(d_bgr)
    s_dev = pipeline.segmentation_sequence_dev(d_bgr, gt, stack, cfg, ctx=ctx)
    s_host = pipeline.segmentation_sequence_dev(d_bgr, gt, host_stack, cfg, ctx=ctx)
    for got, want in ((p_dev, p_host), (s_dev, s_host)):
        assert got.keys() == want.keys()
        for key, v in want.items():
            if isinstance(v, torch.Tensor):
                assert torch.equal(got[key], v), key
            else:
                assert got[key] == v, key
    assert any(len(r) for r in p_dev["rects"])          # some pair is gated: the ROI path ran
    assert np.array_equal(stack.cpu().numpy(), cur_host)   # the stack was read, not written


def test_refusals(nsof_lib, ctx, torch_dev):
    import torch
    from nsof import _lib, frames
    lib = _lib.load()
    src = torch.zeros((2, 32, 32), dtype=torch.uint8, device=torch_dev)
    buf, out = _guarded(torch, torch_dev, (2, 4, 4))
    wy, iy = frames._contributions(32, 4, 4 / 32)
    iy = np.ascontiguousarray(iy, np.int32)
    taps = wy.shape[1]
    torch.cuda.synchronize(torch_dev)

    def call(n_frames=2, width=32, height=32, out_w=4, out_h=4, wts_y=wy.ctypes.data, ind_y=iy.ctypes.data, taps_y=taps,
             wts_x=wy.ctypes.data, taps_x=taps):
        return lib.nsof_frames_compress_u8_dev(ctx.ptr, n_frames, src.data_ptr(), 32, 32 * 32, width, height, out_w, out_h,
                                               wts_y, ind_y, taps_y, wts_x, iy.ctypes.data, taps_x, out.data_ptr())
    assert call(width=3, out_w=4) == _lib.NSOF_EUNSUPPORTED        # an upscale
    assert call(height=2, out_h=4) == _lib.NSOF_EUNSUPPORTED
    assert call(out_w=0) == _lib.NSOF_EINVAL                       # an empty output
    assert call(out_h=0) == _lib.NSOF_EINVAL
    assert call(wts_y=None) == _lib.NSOF_EINVAL                    # null tables
    assert call(ind_y=None) == _lib.NSOF_EINVAL
    assert call(wts_x=None) == _lib.NSOF_EINVAL
    assert call(n_frames=0) == _lib.NSOF_EINVAL
    assert call(taps_y=0) == _lib.NSOF_EINVAL
    assert call(height=16) == _lib.NSOF_EINVAL                     # the tables index rows the frame does not have
    assert lib.nsof_accum_frames_f64_dev(ctx.ptr, out.data_ptr(), 0, 4, 4, 5e-4, 10, 0.7, 1.5, 1.0, out.data_ptr(),
                                         out.data_ptr(), None) == _lib.NSOF_EINVAL
    assert lib.nsof_accum_frames_f64_dev(ctx.ptr, None, 2, 4, 4, 5e-4, 10, 0.7, 1.5, 1.0, out.data_ptr(), out.data_ptr(),
                                         None) == _lib.NSOF_EINVAL

    def status(fn, *args, **kw):
        with pytest.raises(nsof_lib.error) as e:
            fn(*args, out=out, ctx=ctx, **kw)
        assert isinstance(e.value, ValueError)
        return e.value.status
    assert status(frames.process_images_dev, src.cpu(), 8, 8) == _lib.NSOF_EINVAL            # a host tensor
    assert status(frames.process_images_dev, src.float(), 8, 8) == _lib.NSOF_EINVAL          # a float tensor
    assert status(frames.process_images_dev, src, 8, 8, (1, 2), (32, 33)) == _lib.NSOF_ESHAPE   # a crop past the frame
    assert status(frames.process_images_dev, src, 8, 8, (0, 1), (32, 32)) == _lib.NSOF_ESHAPE
    assert status(frames.process_images_dev, src, 64, 8) == _lib.NSOF_ESHAPE                 # an empty grid
    with pytest.raises(nsof_lib.error):
        nsof_lib.simulate_frames_dev(out.float(), ctx=ctx)
    ctx.synchronize()
    assert (buf.cpu().numpy() == SENTINEL).all()                    # nothing was launched
    assert lib.nsof_last_error(ctx.ptr)
