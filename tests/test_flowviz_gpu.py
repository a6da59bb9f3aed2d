"""GPU: the Middlebury colour coding on the device (``nsof_flow_to_image_dev``, ``flowviz.flow_to_image_dev``) against the
reference's goldens, the correctly-rounded host definition of tests/test_flowviz_cpu.py and the NumPy mirror
``nsof.flow_to_image``; per-item normalisation, signs and signed zeros, ``max_flow``, strided views, the prediction
experiment's ``viz_mem`` / ``viz_orig`` and ``save_viz``, and argument checks that launch nothing."""
import numpy as np
import pytest

from test_flowviz_cpu import cr_flow_to_image, golden_cases

pytestmark = pytest.mark.gpu


def _dev(ctx, flows, **kw):
    """flow_to_image_dev on an uploaded copy of host flows -> host uint8 images."""
    import torch
    from nsof import flowviz
    t = torch.from_numpy(np.ascontiguousarray(flows)).cuda()
    torch.cuda.synchronize()
    out = flowviz.flow_to_image_dev(t, ctx=ctx, **kw)
    ctx.synchronize()
    return out.cpu().numpy()


def test_goldens_byte_for_byte(nsof_lib, ctx, torch_dev):
    import torch
    from nsof.errors import NsofValueError
    for name, g in golden_cases().items():
        if name == "f64":
            with pytest.raises(NsofValueError):
                nsof_lib.flow_to_image_dev(torch.from_numpy(g["flow"]).to(torch_dev), ctx=ctx)
            continue
        assert np.array_equal(_dev(ctx, g["flow"]), g["rgb"]), name
        assert np.array_equal(_dev(ctx, g["flow"], convert_to_bgr=True), g["bgr"]), name
        assert np.array_equal(_dev(ctx, g["flow"], clip_flow=2.5), g["clip"]), name


def test_each_item_normalised_by_its_own_max(nsof_lib, ctx, torch_dev):
    import torch
    rng = np.random.default_rng(3)
    scales = (1e-2, 1e-1, 1.0, 1e1, 1e2)
    flows = np.stack([(rng.standard_normal((29, 45, 2)) * s).astype(np.float32) for s in scales])
    t = torch.from_numpy(flows).to(torch_dev)
    norms_dev = torch.full((5,), -1.0, dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    batch = nsof_lib.flow_to_image_dev(t, norms=norms_dev, ctx=ctx)
    ctx.synchronize()
    batch, norms = batch.cpu().numpy(), norms_dev.cpu().numpy()
    assert batch.shape == (5, 29, 45, 3) and batch.dtype == np.uint8
    for k in range(5):
        u, v = flows[k, ..., 0], flows[k, ..., 1]
        div = np.max(np.sqrt(np.square(u) + np.square(v))) + np.float32(1e-5)
        assert div.dtype == np.float32 and norms[k] == div, (k, norms[k], div)
        assert np.array_equal(batch[k], _dev(ctx, flows[k])), k
        assert np.array_equal(batch[k], cr_flow_to_image(flows[k])), k
    # max_flow: the divisor is float32(max_flow + 1e-5) for every item
    nsof_lib.flow_to_image_dev(t, max_flow=3.0, norms=norms_dev, ctx=ctx)
    ctx.synchronize()
    assert (norms_dev.cpu().numpy() == np.float32(3.0 + 1e-5)).all()


def _zero_field():
    """u and v over every combination of +-0, +-tiny and +-large."""
    vals = np.array([0.0, -0.0, 1e-6, -1e-6, 1e3, -1e3], np.float32)
    u, v = np.meshgrid(vals, vals)
    return np.stack([u, v], -1).astype(np.float32)


def test_sign_and_signed_zeros(nsof_lib, ctx, torch_dev):
    import torch
    noise = golden_cases()["noise"]["flow"]
    t = torch.from_numpy(noise).to(torch_dev)
    torch.cuda.synchronize()
    a = nsof_lib.flow_to_image_dev(t, sign=-1, ctx=ctx)
    b = nsof_lib.flow_to_image_dev(-t, ctx=ctx)
    ctx.synchronize()
    assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    f = _zero_field()
    assert np.signbit(f[..., 0]).any() and np.signbit(f[..., 1]).any()
    for clip in (None, 2.5, 0.0):
        for sign in (1, -1):
            host = (-f if sign < 0 else f).astype(np.float32)
            got = _dev(ctx, f, sign=sign, clip_flow=clip)
            assert np.array_equal(got, nsof_lib.flow_to_image(host, clip_flow=clip)), (clip, sign)
            assert np.array_equal(got, cr_flow_to_image(host, clip_flow=clip)), (clip, sign)
    # atan2(+-0, negative) = +-pi: wheel entries 54 and 0 differ, so -0.0 must survive the sign flip and the clip
    img = _dev(ctx, np.array([[[1.0, 0.0], [1.0, -0.0]]], np.float32))
    assert not np.array_equal(img[0, 0], img[0, 1])


def test_max_flow(nsof_lib, ctx, torch_dev):
    g = golden_cases()
    for name in ("smooth", "noise", "tiny", "zero"):
        for mf in (0.0, 0.5, 3.0):
            got = _dev(ctx, g[name]["flow"], max_flow=mf)
            assert np.array_equal(got, nsof_lib.flow_to_image(g[name]["flow"], max_flow=mf)), (name, mf)
            assert np.array_equal(got, cr_flow_to_image(g[name]["flow"], max_flow=mf)), (name, mf)
    f = _zero_field()
    for mf in (0.0, 0.5, 3.0):
        assert np.array_equal(_dev(ctx, f, max_flow=mf, clip_flow=2.5), nsof_lib.flow_to_image(f, 2.5, max_flow=mf))


def test_1080p_farneback_flow(nsof_lib, ctx, torch_dev):
    from nsof import farneback
    from nsof import workload as wl
    prev, nxt = wl.synthetic_sequence(11, 2, 1080, 1920)
    flow = nsof_lib.calcOpticalFlowFarneback(prev, nxt, None, **farneback.PARAMS_A.as_kwargs(), ctx=ctx)
    assert flow.shape == (1080, 1920, 2) and np.abs(flow).max() > 0.5
    for kw in (dict(), dict(convert_to_bgr=True, sign=-1)):
        got = _dev(ctx, flow, **kw)
        host = -flow if kw.get("sign") == -1 else flow
        want = cr_flow_to_image(host, convert_to_bgr=kw.get("convert_to_bgr", False))
        assert np.array_equal(got, want)
        # the NumPy mirror rounds its float32 arctan2 differently now and then (depending on the host's SIMD dispatch):
        # one level on 53 of these 2.07 M pixels in one run, so the bound is 1e-4 of the pixels
        mirror = nsof_lib.flow_to_image(host, convert_to_bgr=kw.get("convert_to_bgr", False))
        diff = np.abs(got.astype(np.int16) - mirror).max(-1)
        assert diff.max() <= 1 and np.count_nonzero(diff) <= 1e-4 * diff.size, (diff.max(), np.count_nonzero(diff))


@pytest.mark.parametrize("x_off", [5, 4])   # 8-byte aligned rows (scalar loads) and 16-byte aligned rows (float4 loads)
def test_strided_views_touch_only_the_crop(nsof_lib, ctx, torch_dev, x_off):
    import torch
    rng = np.random.default_rng(x_off)
    n, h, w = 3, 21, 37
    canvas = (rng.standard_normal((n, h + 10, w + 21, 2)) * 3).astype(np.float32)
    flows = torch.from_numpy(canvas).to(torch_dev)[:, 3:3 + h, x_off:x_off + w]
    out_canvas = torch.full((n, h + 6, w + 7, 3), 77, dtype=torch.uint8, device=torch_dev)
    out = out_canvas[:, 2:2 + h, 3:3 + w]
    norms = torch.zeros((n,), dtype=torch.float32, device=torch_dev)
    torch.cuda.synchronize()
    assert not flows.is_contiguous() and not out.is_contiguous()
    ret = nsof_lib.flow_to_image_dev(flows, out, clip_flow=None, convert_to_bgr=True, norms=norms, ctx=ctx)
    ctx.synchronize()
    assert ret is out
    oc = out_canvas.cpu().numpy()
    for k in range(n):
        want = cr_flow_to_image(canvas[k, 3:3 + h, x_off:x_off + w], convert_to_bgr=True)
        assert np.array_equal(oc[k, 2:2 + h, 3:3 + w], want), k
    mask = np.ones(oc.shape, bool)
    mask[:, 2:2 + h, 3:3 + w] = False
    assert (oc[mask] == 77).all()
    # one flow [H][W][2] -> one image [H][W][3], also into a strided view
    one = nsof_lib.flow_to_image_dev(flows[1], out_canvas[1, 2:2 + h, 3:3 + w], ctx=ctx)
    ctx.synchronize()
    assert one.shape == (h, w, 3)
    assert np.array_equal(one.cpu().numpy(), cr_flow_to_image(canvas[1, 3:3 + h, x_off:x_off + w]))


def test_prediction_sequence_viz_and_save_viz(nsof_lib, ctx, torch_dev, tmp_path):
    pil = pytest.importorskip("PIL.Image")
    import torch
    from nsof import flowviz, pipeline
    from test_predict_sequence import SMALL, _grasp_json_stack, _synthetic_bgr
    stack = _grasp_json_stack()
    h, w = stack.shape[0] * 16, stack.shape[1] * 16
    frames = _synthetic_bgr(5, 4, h, w)
    d = torch.from_numpy(np.stack(frames)).to(torch_dev)
    torch.cuda.synchronize()
    cfg = lambda: nsof_lib.dataset_config("grasp", **SMALL)  # noqa: E731
    base = pipeline.prediction_sequence_dev(d, stack, cfg(), ctx=ctx)
    res = pipeline.prediction_sequence_dev(d, stack, cfg(), ctx=ctx, with_viz=True)
    assert set(res) == set(base) | {"viz_mem", "viz_orig"}
    for key, val in base.items():
        if isinstance(val, torch.Tensor):
            assert torch.equal(res[key], val), key
        else:
            assert res[key] == val, key
    n_pairs = len(frames) - 2
    for path in ("mem", "orig"):
        viz, flow = res[f"viz_{path}"].cpu().numpy(), res[f"flow_{path}"].cpu().numpy()
        assert viz.shape == (n_pairs, h, w, 3) and viz.dtype == np.uint8
        for k in range(n_pairs):
            assert np.array_equal(viz[k], cr_flow_to_image(-flow[k], convert_to_bgr=True)), (path, k)
        ours = [str(tmp_path / f"{path}_dev_{k}.png") for k in range(n_pairs)]
        flowviz.save_viz(res[f"viz_{path}"], ours)
        for k in range(n_pairs):
            theirs = str(tmp_path / f"{path}_host_{k}.png")
            nsof_lib.viz(-flow[k], theirs)
            mine, host = np.asarray(pil.open(ours[k])), np.asarray(pil.open(theirs))
            assert np.array_equal(mine, viz[k]), (path, k)
            # equal wherever the mirror's float32 arctan2 rounds as the device does (all but about 1e-5 of the pixels)
            same = (nsof_lib.flow_to_image(-flow[k], convert_to_bgr=True) == viz[k]).all(-1)
            assert np.array_equal(mine[same], host[same]), (path, k)
            assert np.count_nonzero(~same) <= 1e-4 * same.size, (path, k)
            assert np.abs(mine.astype(np.int16) - host).max() <= 1, (path, k)
    no_orig = pipeline.prediction_sequence_dev(d, stack, cfg(), with_original=False, ctx=ctx, with_viz=True)
    assert no_orig["viz_orig"] is None and torch.equal(no_orig["viz_mem"], res["viz_mem"])


def test_argument_errors_launch_nothing(nsof_lib, torch_dev):
    import torch
    from nsof import _lib
    from nsof.errors import NsofValueError
    c = nsof_lib.Context(0)
    try:
        fl = torch.ones((2, 8, 12, 2), dtype=torch.float32, device=torch_dev)
        out = torch.full((2, 8, 12, 3), 7, dtype=torch.uint8, device=torch_dev)
        norms = torch.full((2,), 5.0, dtype=torch.float32, device=torch_dev)
        torch.cuda.synchronize()
        for bad in (dict(flows=fl.double()), dict(flows=fl.cpu()), dict(flows=fl.cpu().numpy()),
                    dict(flows=torch.ones((2, 8, 12, 3), dtype=torch.float32, device=torch_dev)),
                    dict(clip_flow=-1.0), dict(max_flow=-0.5), dict(max_flow=float("nan")), dict(sign=0),
                    dict(out=out[:1]), dict(out=out.float()), dict(norms=norms[:1])):
            kw = dict(flows=fl, out=out, norms=norms)
            kw.update(bad)
            with pytest.raises(NsofValueError):
                nsof_lib.flow_to_image_dev(kw.pop("flows"), ctx=c, **kw)
        L = c._lib

        def call(n=2, f=fl.data_ptr(), rs=24, is_=192, w=12, h=8, sign=1, o=out.data_ptr(), ors=36, ois=288):
            return L.nsof_flow_to_image_dev(c.ptr, n, f, rs, is_, w, h, sign, -1.0, -1.0, 0, o, ors, ois,
                                            norms.data_ptr())
        assert call() == _lib.NSOF_OK        # the arguments below differ from a valid call in one place each
        c.synchronize()
        out.fill_(7)
        norms.fill_(5.0)
        torch.cuda.synchronize()
        for bad in (dict(n=0), dict(w=0), dict(h=-1), dict(f=None), dict(o=None), dict(rs=23), dict(ors=35),
                    dict(is_=24 * 7 + 23), dict(ois=36 * 7 + 35), dict(is_=-192), dict(sign=0), dict(sign=2)):
            assert call(**bad) == _lib.NSOF_EINVAL, bad
        c.synchronize()
        assert (out.cpu() == 7).all() and (norms.cpu() == 5.0).all()
    finally:
        c.close()
