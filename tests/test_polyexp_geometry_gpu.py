"""GPU parity of the exact polynomial expansion (k_polyexp_rs) at the launch geometries the bit-exact stage test does not
reach: the full 1920-column width over enough images for several rounds of workgroups per CU, widths that are not a
multiple of the strip width or of 4, heights that end inside a 4-row step or a row segment, heights below 4, and every
radius N = 1..10.  R must equal the oracle's bit for bit.

The level-0 form that builds the image from the 8-bit frame inside the expansion (k_polyexp_rs<.., U8>) has no stage
entry of its own: it is checked through the batch entry and the work-list entry, whose flows in the exact order equal
the oracle's pyramid + expansion + iteration bit for bit."""
import numpy as np
import pytest

from conftest import ulp_diff

pytestmark = pytest.mark.gpu

NS = [(1, 1.05), (2, 0.9), (3, 1.1), (4, 0.8), (5, 1.2), (6, 1.3), (7, 1.5), (8, 1.6), (9, 1.8), (10, 1.05)]


def _rlayout(aos):
    """Oracle R (h,w,5) -> device layout of one image: [h][w][4] (channels 0..3) then [h][w] (channel 4), flat."""
    return np.concatenate([np.ascontiguousarray(aos[..., :4]).ravel(), np.ascontiguousarray(aos[..., 4]).ravel()])


def _check_stage(ctx, oracle, torch_dev, imgs, n, sigma):
    import torch
    k, h, w = imgs.shape
    d = torch.from_numpy(np.ascontiguousarray(imgs)).to(torch_dev)
    out = torch.full((k, 5 * h * w), float("nan"), dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    ctx.check(ctx._lib.nsof_stage_polyexp(ctx.ptr, k, d.data_ptr(), w, h, n, sigma, out.data_ptr()))
    ctx.synchronize()
    got = out.cpu().numpy()
    for i in range(k):
        want = _rlayout(oracle.polyexp(imgs[i], n, sigma))
        assert np.array_equal(got[i], want), f"N={n} {h}x{w} image {i}: max ulp {ulp_diff(got[i], want).max()}"


@pytest.mark.parametrize("n,sigma", NS)
@pytest.mark.parametrize("shape", [(37, 241), (61, 483), (130, 1023), (3, 250), (2, 1), (1, 7), (258, 17)])
def test_polyexp_odd_shapes_bit_exact(ctx, oracle, torch_dev, n, sigma, shape):
    rng = np.random.default_rng(n * 7919 + shape[0] * 31 + shape[1])
    imgs = (rng.random((3,) + shape) * 255).astype(np.float32)
    imgs[1] = np.add.outer(np.arange(shape[0]) * 3.0, np.arange(shape[1]) * 0.5).astype(np.float32) % 255   # ramps
    _check_stage(ctx, oracle, torch_dev, imgs, n, sigma)


@pytest.mark.parametrize("n,sigma", [(5, 1.2), (1, 1.05), (10, 1.05)])
def test_polyexp_full_width_many_rounds(ctx, oracle, torch_dev, n, sigma):
    """1920 columns, 96 images: 1536 workgroups or more, more than a round of 4 per CU on every CU."""
    rng = np.random.default_rng(n)
    imgs = (rng.random((96, 134, 1920)) * 255).astype(np.float32)
    _check_stage(ctx, oracle, torch_dev, imgs, n, sigma)


def test_polyexp_full_frame(ctx, oracle, torch_dev):
    """1080 x 1920 (the bench's level 0, row segments of more than one step)."""
    rng = np.random.default_rng(1080)
    imgs = (rng.random((4, 1080, 1920)) * 255).astype(np.float32)
    _check_stage(ctx, oracle, torch_dev, imgs, 5, 1.2)


def _u8_frames(seed, h, w):
    from nsof import synth
    return synth.make_pair(seed, h, w)


@pytest.mark.parametrize("params", [(0.5, 3, 15, 3, 5, 1.2, 0), (0.6, 3, 3, 3, 10, 1.05, 0), (0.6, 3, 4, 2, 1, 1.05, 0),
                                    (0.5, 2, 7, 2, 7, 1.5, 0)])
def test_polyexp_u8_level0_batch_and_worklist(nsof_lib, ctx, oracle, params):
    """The 8-bit level-0 expansion through the batch entry (one shape, several pairs) and the work-list entry (mixed
    shapes: odd widths, heights ending mid-step, a frame narrower than one strip)."""
    import torch
    h, w = 67, 503
    pairs = [_u8_frames(11 + i, h, w) for i in range(3)]
    P = nsof_lib.FarnebackParams(*params)
    dev = torch.device("cuda", 0)
    dp = torch.from_numpy(np.stack([p for p, _ in pairs])).to(dev)
    dn = torch.from_numpy(np.stack([q for _, q in pairs])).to(dev)
    fb = torch.empty((len(pairs), h, w, 2), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    nsof_lib.farneback_batch(dp, dn, fb, len(pairs), h, w, P, ctx=ctx)
    ctx.synchronize()
    got = fb.cpu().numpy()
    for i, (p, q) in enumerate(pairs):
        want = oracle.farneback(p, q, *params)
        assert np.array_equal(got[i], want), ("batch", i, float(np.abs(got[i] - want).max()))

    mixed = [_u8_frames(40 + i, hh, ww) for i, (hh, ww) in enumerate([(45, 250), (130, 481), (33, 97), (71, 1921)])]
    flows = nsof_lib.farneback_pairs(mixed, P, ctx=ctx)
    for i, (p, q) in enumerate(mixed):
        want = oracle.farneback(p, q, *params)
        assert np.array_equal(flows[i], want), ("work list", i, p.shape, float(np.abs(flows[i] - want).max()))
