"""CPU: what the references make of the fields of tests/heads_nonfinite_cases.py, before any kernel is compared with them
(tests/test_heads_nonfinite_gpu.py): the fields hold what they claim to hold, the colour reference keeps ordinary colours
beside NaN pixels and whitens everything beside an infinite one, the oracle's remap samples at INT_MIN for every special
flow value, its mask threshold is the float64 one, and the float-frame Farneback flow of part 3 is NaN on more than a
fifth of its pixels and finite on more than a fifth."""
import numpy as np
import pytest

import heads_nonfinite_cases as K
from test_flowviz_cpu import cr_flow_to_image_nonfinite
from test_nonfinite_cpu import REMAP_BAD


def _holds(flow, value):
    if value != value:
        return np.isnan(flow)
    return (flow == np.float32(value)) & (np.signbit(flow) == np.signbit(np.float32(value)))


def test_fields_hold_every_special_in_u_in_v_and_in_both():
    flow = K.warp_flow(301)
    for s in K.SINGLES + K.WARP_EXTRA:
        m = _holds(flow, s)
        assert (m[..., 0] & ~m[..., 1]).any() and (~m[..., 0] & m[..., 1]).any() and m.all(-1).any(), s
    for a, b in K.PAIRS:
        assert (_holds(flow[..., 0], a) & _holds(flow[..., 1], b)).any(), (a, b)
        assert (_holds(flow[..., 0], b) & _holds(flow[..., 1], a)).any(), (a, b)
    assert np.float32(1e-40) != 0 and np.float32(1e-40) < np.finfo(np.float32).tiny          # a float32 subnormal
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(2.0 ** 64) * np.float32(2.0 ** 64)) and np.isinf(np.float32(3e38) * np.float32(3e38))
    # corners, edges and interior all carry one, and so does every rectangle of the warp tests
    bad = ~np.isfinite(flow).all(-1) | (np.abs(flow) > 1e9).any(-1)
    bad |= _holds(flow, 1e-40).any(-1) | _holds(flow, -0.0).any(-1)
    h, w = bad.shape
    assert bad[0, 0] and bad[0, w - 1] and bad[h - 1, 0] and bad[h - 1, w - 1] and bad[1:-1, 1:-1].sum() >= 20
    for x0, y0, x1, y1 in K.WARP_RECTS:
        assert bad[y0:y1, x0:x1].any()
    for k, (counts, rects) in enumerate(zip(K.SEQ_COUNTS, K.SEQ_RECTS)):
        for x0, y0, x1, y1 in rects[:counts]:
            assert bad[y0:y1, x0:x1].any(), k


def test_colour_reference_on_the_three_fields(nsof_lib):
    f = K.colour_fields()
    assert np.isnan(f["nan"]).any() and not np.isinf(f["nan"]).any() and np.isfinite(f["finite"]).all()
    assert np.isinf(f["inf"]).any() and np.isnan(f["inf"]).any()
    for sign in (1, -1):
        img, d = cr_flow_to_image_nonfinite(np.float32(sign) * f["nan"])
        nan = np.isnan(f["nan"]).any(-1)
        assert np.isfinite(d) and d > 2 and (img[nan] == 0).all() and (img[~nan] != 0).any(-1).all()
        assert len(np.unique(img.reshape(-1, 3), axis=0)) > 50
        img, d = cr_flow_to_image_nonfinite(np.float32(sign) * f["inf"])
        with np.errstate(over="ignore", invalid="ignore"):
            mag = np.sqrt(np.square(f["inf"][..., 0]) + np.square(f["inf"][..., 1]))
        assert np.isposinf(d)
        black = ~np.isfinite(f["inf"]).all(-1)                # inf / inf and NaN; a finite 3e38 / inf is 0 like the rest
        assert (img[~black] == 255).all() and (img[black] == 0).all()
        assert (np.isfinite(f["inf"]).all(-1) & np.isinf(mag)).any()          # a finite pixel whose magnitude overflows
        for mf in (0.5, 3.0):
            img, d = cr_flow_to_image_nonfinite(np.float32(sign) * f["inf"], max_flow=mf)
            inf_px = np.isinf(f["inf"]).any(-1) & ~np.isnan(f["inf"]).any(-1)
            assert d == np.float32(mf + 1e-5) and (img[inf_px] != 0).any(-1).all() and (img[inf_px] <= 191).all()
            assert (img[np.isnan(f["inf"]).any(-1)] == 0).all()
        # the clip turns +inf into 2.5 and -inf into +0 and keeps NaN: a finite divisor again
        img, d = cr_flow_to_image_nonfinite(np.float32(sign) * f["inf"], clip_flow=2.5)
        assert d == np.float32(np.float32(np.sqrt(np.float32(12.5))) + np.float32(1e-5))
        assert np.array_equal((img == 0).all(-1), np.isnan(f["inf"]).any(-1))
    for h, w in K.COLOUR_SHAPES:
        s = K.shape_field(h, w)
        assert s.shape == (h, w, 2) and np.isnan(s[h - 1]).any() and np.isnan(s[:, w - 1]).any()
        img, d = cr_flow_to_image_nonfinite(s)
        assert np.isfinite(d) and np.array_equal((img == 0).all(-1), np.isnan(s).any(-1))


@pytest.mark.parametrize("border", [0, 1])
def test_oracle_remap_of_the_special_maps(oracle, border):
    """Every special value, used as a map coordinate, is NaN, infinite or beyond the int range after x32 (INT_MIN: the
    tap lands at -32768), or rounds to +-0 (the subnormal, -0.0): the source's first column / row exactly."""
    rng = np.random.default_rng(4)
    bad = REMAP_BAD + [2.0 ** 26 - 4]
    for (sh, sw), cn in [((9, 13), 1), ((9, 13), 3)] + [(s, 3) for s in K.REMAP_SOURCES_3CH]:
        src = rng.integers(1, 255, (sh, sw) if cn == 1 else (sh, sw, cn), dtype=np.uint8)
        mx, my = K.remap_maps(sw, sh, bad, default=(0.0, 0.0))
        got = oracle.remap_linear(src, mx, my, border, 7)
        n = len(REMAP_BAD)
        if border == 0:
            assert (got[:3, :n] == 7).all()
        else:
            assert (got[0, :n] == src[0, 0]).all() and (got[1, :n] == src[0, 0]).all() and (got[2, :n] == src[0, 0]).all()
            assert (got[2, n] == src[-1, -1]).all()
    flow = K.warp_flow(301)
    src = rng.integers(1, 255, (K.H, K.W, 3), dtype=np.uint8)
    for sign in (1, -1):
        mx, my = oracle.flow_map(flow, (0, 0, K.W, K.H), sign)
        got = oracle.remap_linear(src, mx, my, border)
        with np.errstate(invalid="ignore"):
            far = ~np.isfinite(flow) | (np.abs(flow) > 1e9)
        gone = far[..., 0] | far[..., 1]
        assert gone.sum() >= 30
        if border == 0:
            assert (got[gone] == 0).all()
        both = far.all(-1)
        if border == 1:
            assert (got[both] == src[0, 0]).all()          # INT_MIN on both axes: the top-left pixel, whatever the sign
        # the subnormal and -0.0 move nothing: the map is the grid there
        for s in (1e-40, -0.0):
            still = _holds(flow, s).all(-1)
            assert still.any() and np.array_equal(got[still], src[still])


def test_oracle_mask_threshold_is_the_float64_one(oracle):
    for flow, marks in K.mask_flows():
        m0 = oracle.motion_mask(flow, 1.0, 10, 0)
        assert np.array_equal(m0, K.float64_mask(flow))
        nan = np.isnan(flow).any(-1)
        inf = np.isinf(flow).any(-1) & ~nan
        big = (np.abs(flow) == np.float32(3e38)).any(-1) & ~nan
        assert nan.sum() >= 5 and inf.sum() >= 8 and big.sum() >= 6
        assert not m0[nan].any() and m0[inf].all() and m0[big].all()
        for name, (vec, moves) in K.MASK_MARKS.items():
            y, x = marks[name]
            assert flow[y, x].tolist() == [np.float32(vec[0]), np.float32(vec[1])]
            assert m0[y, x] == (255 if moves else 0), name
            if name.startswith("lone"):                      # isolated: its 8 neighbours do not move
                assert m0[y - 1:y + 2, x - 1:x + 2].sum() == 255, name
        # the marks a float32 magnitude gets wrong are wrong in float32 indeed
        for name in ("six_eight", "f32_rounds_down_a", "f32_rounds_down_b"):
            u, v = (np.float32(c) for c in K.MASK_MARKS[name][0])
            assert not np.sqrt(u * u + v * v) > np.float32(1.0), name
        for iters, ksize in K.MASK_CHAINS:
            m = oracle.motion_mask(flow, 1.0, ksize, iters)
            assert set(np.unique(m).tolist()) == {0, 255}, (iters, ksize)
        assert not np.array_equal(oracle.motion_mask(flow, 1.0, 10, 5), m0)       # the closing does something
        # a threshold above float32's range: the overflowing finites stay below it in float64, the infinities do not
        m39 = oracle.motion_mask(flow, 1e39, 10, 0)
        assert np.array_equal(m39, K.float64_mask(flow, 1e39)) and np.array_equal(m39 != 0, inf)
        for k, boxes in enumerate(K.MASK_BOXES):
            for x0, y0, x1, y1 in boxes:
                crop = oracle.motion_mask(np.ascontiguousarray(flow[y0:y1, x0:x1]), 1.0, 10, 5)
                assert set(np.unique(crop).tolist()) == {0, 255}, (k, x0, y0)


def test_farneback_flow_of_part_3_is_partly_nan(oracle):
    """Condition, not measurement: each kind of pixel is more than a fifth of the frame, so neither is the part the GPU
    test says nothing about."""
    _, _, flow = K.farneback_nan_case(oracle)
    nan = np.isnan(flow).any(-1)
    finite = np.isfinite(flow).all(-1)
    assert flow.shape == (64, 96, 2) and flow.dtype == np.float32
    assert nan.mean() >= 0.20 and finite.mean() >= 0.20, (nan.mean(), finite.mean())
    mask = oracle.motion_mask(flow, 1.0, 10, 0)
    assert np.array_equal(mask, K.float64_mask(flow)) and 0 < (mask != 0).mean() < 1
    img, d = cr_flow_to_image_nonfinite(flow)
    assert np.isfinite(d) and np.array_equal((img == 0).all(-1), nan)
    assert len(np.unique(img.reshape(-1, 3), axis=0)) > 50
