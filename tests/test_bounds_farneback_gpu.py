"""GPU: the Farneback entries write only their outputs and read only their inputs (include/nsof.h, "Layout rule").

Every case runs its entry TWICE, with two different poisons around the inputs (tests/guard_bands.py: band, row padding,
padding between images), each time into a fresh output inside a guard band, and asserts

  (a) both outputs equal the CPU reference the existing stage tests use -- ``oracle.*``, ``pyr_level_f32`` of
      tests/test_float_reference.py for frames that are not 8-bit -- bit for bit (the two inexact modes named below keep
      the bound the project derives for them); the library's own dense call is never the reference;
  (b) the two runs equal each other bit for bit: a result that moves with the poison was computed from memory outside
      the frame (a NaN that arrives through a zero-weight multiply included);
  (c) every byte outside the logical elements of the output still holds the band pattern.

Poisons: 8-bit frames 0x00 / 0xFF; 16-bit frames 0x0000 / 0x8000 (uint16) and 0x0000 / 0x7FFF (int16); float inputs
(f32 frames, R, M, flow) a quiet NaN / +-1e30.  Every case runs with one image and with two: with one, an overrun between
images shows in the band; with two, the second input sits behind poisoned padding.

Outputs of the stage entries are dense and are handed over 256-byte aligned, as the driver's workspace hands them over
(the kernels' vector stores assume the alignment of their launch's first element); the INPUT frames are the ones that
arrive at any element, with any padding, so offsets and ragged pitches are applied to them.
"""
import ctypes as C

import numpy as np
import pytest

import farneback_f64 as F
import farneback_gauss as FG
from guard_bands import banded_out, surrounded_in
from test_farneback_f64 import _stage_inputs
from test_farneback_gpu import SHORT_CASES, _planar, _rlayout
from test_float_reference import farneback_f32, pyr_level_f32

pytestmark = pytest.mark.gpu

QNAN = np.float32(np.nan)
FLOAT_POISONS = (QNAN, np.float32(-1e30))
# dtype -> (nsof_pixel_type, poison A, poison B, frame of that type from 8-bit noise: the 16-bit ones fill their range)
PIXEL_TYPES = {
    "uint8": (0, 0x00, 0xFF, lambda a: a),
    "float32": (1, QNAN, np.float32(1e30), lambda a: (a.astype(np.float32) * np.float32(3.7) - np.float32(300.0))),
    "uint16": (2, 0x0000, 0x8000, lambda a: (a.astype(np.uint16) * np.uint16(257))),
    "int16": (3, 0x0000, 0x7FFF, lambda a: (a.astype(np.int32) * 257 - 32768).astype(np.int16)),
}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 2: np.uint16, 1: np.uint8}[a.dtype.itemsize])


def _judge(what, runs, wants, tol=None):
    """runs: [(got, check)] of the two poisons; wants: the reference, or None where only (b) and (c) apply.  All three
    assertions are evaluated before any is raised, so that a failure reports everything it shows."""
    errs = []
    for k, (got, check) in enumerate(runs):
        if wants is not None:
            want = np.ascontiguousarray(wants, np.float32) if got.dtype == np.float32 else wants
            if got.shape != want.shape:
                errs.append(f"(a) run {k}: shape {got.shape}, reference {want.shape}")
            elif tol is not None:
                ok, worst = F.within(got, want, tol)
                if not ok:
                    errs.append(f"(a) run {k}: {worst:.3g} x the derived bound from the reference")
            elif not np.array_equal(_bits(got), _bits(want)):
                bad = np.argwhere(_bits(got) != _bits(want))
                errs.append(f"(a) run {k}: {len(bad)} of {got.size} values differ from the reference, first at "
                            f"{tuple(bad[0])}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}")
        try:
            check()
        except AssertionError as e:
            errs.append(f"(c) run {k}: {e}")
    if not np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])):
        bad = np.argwhere(_bits(runs[0][0]) != _bits(runs[1][0]))
        errs.append(f"(b) the result depends on the poison around the inputs: {len(bad)} values, first at {tuple(bad[0])}: "
                    f"{runs[0][0][tuple(bad[0])]!r} / {runs[1][0][tuple(bad[0])]!r}")
    assert not errs, f"{what}:\n  " + "\n  ".join(errs)


def _noise_u8(seed, n, h, w):
    """n frames of 8-bit noise over a ramp (a reflection error at a border shows on the ramp)."""
    rng = np.random.default_rng(seed)
    ramp = (np.add.outer(np.arange(h) * 5, np.arange(w) * 3) % 120).astype(np.int32)
    return np.stack([(ramp + rng.integers(0, 136, (h, w))).astype(np.uint8) for _ in range(n)])


# ---- 1. nsof_stage_pyr_level_px ----------------------------------------------------------------------------------------
# How the input frames sit in memory: (pitch_extra, item_extra, offset_elems) in ELEMENTS.
#   vec:   the row pitch is W rounded up to a multiple of 16 elements plus 16, images 32 elements apart, so that rows and
#          images stay aligned for every vector form (16 elements = 16 bytes at least)
#   rag13: the padding the existing stage tests use (13), images 7 elements apart, start aligned
#   rag5:  another ragged pitch and a start one element past the aligned address: the scalar routes
LAYOUTS = {"vec": (16, 32, 0), "rag13": (13, 7, 0), "rag5": (5, 3, 1)}

# route, (H, W), pyr_scale, level, (wk, hk, taps) that nsof_farneback_level_size must give, layout.
# Outputs per lane (columns) and rows per step of each route, from csrc/farneback_pyramid.hip:
#   k_prep_same3_vec  4 columns per lane (W % 4 == 0 is the route's condition: residue 0 only), PREP0_ROWS = 8 rows per
#                     wave, 4 waves = 32 rows per workgroup: heights 1..9, 31, 32, 33; 260 columns = a second workgroup
#   k_prep_same       1 pixel per thread, 64 x 4 per workgroup: widths 7, 9, 10, 11, 65, heights 1..5
#   k_prep_decim      CWL / S columns per lane (CWL = 16 when W % 16 == 0, else 8: wk is a multiple of it by the
#                     route's condition), U = RING / S rows per unrolled step: U = 2 at S = 2 (hk 2, 3, 4), U = 3 at
#                     S = 4 and 8 (hk 3, 4, 5); launches this small run segments of U rows, so hk = 5 is two segments;
#                     520 and 1040 columns are 65 lanes = a second wave.  f32 at S = 8 with 8-column lanes (W % 16 == 8)
#                     is not a decimation case: the launcher sends it to rows / cols (prep_route: "f32 takes 8-column
#                     lanes only while the blur halo fits in one"), asserted bit for bit like the others
#   k_prep_walk       one column per lane, 64 per wave: wk 5 .. 105; segments of at least 8 rows
#   k_prep_direct     one pixel per thread; only the 3-tap instance is reachable here (direct<5> needs H / hk >= 5 with
#                     5 taps, and a pyr_scale that small has more taps): NO stage case reaches k_prep_direct<5>
#   k_prep_rows/cols  PREPA_ROWS = 8 source rows per wave, 32 per workgroup (H 5, 9, 24 .. 40), one column per lane
#   k_prep_tiled      PREP_TW x PREP_TH = 32 x 8 outputs per workgroup: 39 x 3 and 21 x 12 (partial tiles on both axes)
#   k_prep_naive      one pixel per thread; 8 x 8 is the smallest frame with a level 3 at pyr_scale 0.4 (37 taps, one
#                     output pixel).  The entry refuses pyr_scale >= 1, so the route's upscaling arm has no stage case
PYR_CASES = (
    [("same3_vec", (h, 8), 0.5, 0, (8, h, 3), "vec") for h in range(1, 9)] +
    [("same3_vec", (9, 12), 0.5, 0, (12, 9, 3), "vec"), ("same3_vec", (33, 16), 0.5, 0, (16, 33, 3), "vec"),
     ("same3_vec", (31, 8), 0.5, 0, (8, 31, 3), "vec"), ("same3_vec", (32, 12), 0.5, 0, (12, 32, 3), "vec"),
     ("same3_vec", (3, 260), 0.5, 0, (260, 3, 3), "vec"),
     ("same", (1, 7), 0.5, 0, (7, 1, 3), "rag13"), ("same", (3, 9), 0.5, 0, (9, 3, 3), "rag13"),
     ("same", (5, 10), 0.5, 0, (10, 5, 3), "rag5"), ("same", (2, 11), 0.5, 0, (11, 2, 3), "rag13"),
     ("same", (4, 65), 0.5, 0, (65, 4, 3), "rag5"),
     ("same", (9, 12), 0.5, 0, (12, 9, 3), "rag5"),        # the vector route's shape, one element off its alignment
     ("decim2", (4, 64), 0.5, 1, (32, 2, 3), "vec"), ("decim2", (6, 72), 0.5, 1, (36, 3, 3), "vec"),
     ("decim2", (8, 80), 0.5, 1, (40, 4, 3), "vec"), ("decim2", (4, 1040), 0.5, 1, (520, 2, 3), "vec"),
     ("decim2", (4, 520), 0.5, 1, (260, 2, 3), "vec"),
     ("decim4", (12, 64), 0.5, 2, (16, 3, 9), "vec"), ("decim4", (16, 72), 0.5, 2, (18, 4, 9), "vec"),
     ("decim4", (20, 88), 0.5, 2, (22, 5, 9), "vec"),
     ("decim8", (24, 64), 0.5, 3, (8, 3, 19), "vec"), ("decim8", (32, 72), 0.5, 3, (9, 4, 19), "vec"),
     ("decim8", (40, 128), 0.5, 3, (16, 5, 19), "vec")] +
    [("short", shape, ps, level, geom, lay) for (shape, ps, level, geom) in SHORT_CASES for lay in ("rag13", "rag5")] +
    [("walk3", (12, 200), 0.42, 1, (84, 5, 3), "rag5"), ("walk5", (5, 300), 0.35, 1, (105, 2, 5), "rag13"),
     ("walk9", (21, 203), 0.5, 2, (51, 5, 9), "rag5"),
     ("walk9", (20, 200), 0.5, 2, (50, 5, 9), "rag5"),      # a decimation shape off its alignment
     ("direct3", (3, 150), 0.45, 1, (68, 1, 3), "rag5"),
     ("rows_cols", (40, 300), 0.35, 2, (37, 5, 19), "rag13"),
     ("rows_cols", (24, 64), 0.5, 3, (8, 3, 19), "rag5"),   # a decimation shape off its alignment
     ("tiled", (40, 70), 0.3, 1, (21, 12, 7), "rag5"),
     ("naive", (8, 8), 0.4, 3, (1, 1, 37), "rag13"), ("naive", (30, 30), 0.4, 3, (2, 2, 37), "rag5"),
     ("naive", (20, 40), 0.4, 3, (3, 1, 37), "vec")])
# one case per route in the FMA variant (8-bit frames: the oracle's FMA twin takes those)
PYR_FMA = {("same3_vec", (9, 12)), ("same", (5, 10)), ("decim2", (6, 72)), ("decim4", (20, 88)), ("decim8", (40, 128)),
           ("short", (3, 40)), ("short", (5, 40)), ("short", (9, 130)), ("walk9", (21, 203)), ("direct3", (3, 150)),
           ("rows_cols", (40, 300)), ("tiled", (40, 70)), ("naive", (30, 30))}


def _pyr_id(c):
    return f"{c[0]}-{c[1][0]}x{c[1][1]}-s{c[2]}-l{c[3]}-{c[5]}"


def _pyr_level_case(nsof_lib, ctx, oracle, torch_dev, case, dtypes):
    import torch
    route, (h, w), ps, level, geom, lay = case
    assert nsof_lib.level_size(w, h, ps, level)[:3] == geom
    wk, hk, _ = geom
    pitch_extra, item_extra, offset = LAYOUTS[lay]
    if lay == "vec":
        pitch_extra += (-w) % 16
    base = _noise_u8(h * 1000 + w, 2, h, w)
    for dtype in dtypes:
        pt, poison_a, poison_b, conv = PIXEL_TYPES[dtype]
        frames = np.stack([conv(base[0]), conv(base[1])])
        assert frames.dtype == np.dtype(dtype)
        if dtype == "uint8":
            want = np.stack([oracle.pyr_level(f, ps, level) for f in frames])
        else:
            want = np.stack([pyr_level_f32(oracle, f.astype(np.float32), ps, level) for f in frames])
        assert want.shape == (2, hk, wk)
        for n_img in (1, 2):
            runs = []
            for poison in (poison_a, poison_b):
                src = surrounded_in(torch, torch_dev, frames[:n_img], np.dtype(dtype).type(poison), pitch_extra=pitch_extra,
                                    item_extra=item_extra, offset_elems=offset)
                if lay == "vec":   # what the vector routes ask of the frames: the table's route names depend on it
                    assert src.data_ptr() % 16 == 0 and src.row_stride % 16 == 0 and src.item_stride % 16 == 0
                out, check = banded_out(torch, torch_dev, (n_img, hk, wk), np.float32)
                ctx.check(ctx._lib.nsof_stage_pyr_level_px(ctx.ptr, pt, n_img, src.data_ptr(), src.row_stride, src.item_stride, w,
                                                           h, ps, level, out.data_ptr()))
                ctx.synchronize()
                runs.append((out.cpu().numpy(), check))
            _judge(f"pyr_level {route} {(h, w)} scale {ps} level {level} {dtype} n_img={n_img} {lay}", runs, want[:n_img])


@pytest.mark.parametrize("case", PYR_CASES, ids=[_pyr_id(c) for c in PYR_CASES])
def test_stage_pyr_level_px(nsof_lib, ctx, oracle, torch_dev, case):
    """Every route of the pyramid stage, all four pixel types, plain arithmetic."""
    _pyr_level_case(nsof_lib, ctx, oracle, torch_dev, case, list(PIXEL_TYPES))


@pytest.mark.parametrize("case", [c for c in PYR_CASES if (c[0], c[1]) in PYR_FMA],
                         ids=[_pyr_id(c) for c in PYR_CASES if (c[0], c[1]) in PYR_FMA])
def test_stage_pyr_level_px_fma(nsof_lib, ctx, oracle, torch_dev, case):
    """The FMA twin (NSOF_OPT_PYR_FMA) of every route, against the oracle built with the same switch."""
    from nsof import _lib
    try:
        ctx.set_option(_lib.OPT_PYR_FMA, 1)
        oracle.set_pyr_fma(True)
        _pyr_level_case(nsof_lib, ctx, oracle, torch_dev, case, ["uint8"])
    finally:
        ctx.set_option(_lib.OPT_PYR_FMA, 0)
        oracle.set_pyr_fma(False)


# ---- 2. the other stages ------------------------------------------------------------------------------------------------
def _float_in(torch, torch_dev, arr, poison, row_dims=1, offset=0):
    """A dense float input of a stage entry (these take no strides) in a band of poison."""
    return surrounded_in(torch, torch_dev, np.ascontiguousarray(arr, np.float32), poison, offset_elems=offset,
                         row_dims=row_dims)


# destination (h, w): widths 1, 2, 3, 254, 255 take k_flow_upsample2x2 (a thread per 2 x 2 block: both parities of both
# axes), 256, 257, 258 the row walk (2 columns per lane, UPW_SEG = 32 rows per segment: heights 1, 31, 32, 33)
UPSAMPLE_DST = [(1, 1), (2, 2), (3, 3), (5, 254), (4, 255), (1, 256), (31, 257), (32, 258), (33, 256), (33, 257)]


@pytest.mark.parametrize("pyr_scale", [0.5, 0.6])
@pytest.mark.parametrize("dst", UPSAMPLE_DST + ["down"], ids=[f"{h}x{w}" for h, w in UPSAMPLE_DST] + ["downsampling"])
def test_stage_flow_upsample(ctx, oracle, torch_dev, dst, pyr_scale):
    """The source size is what the coarser level would have (the destination times pyr_scale, rounded); `down` is a
    destination smaller than its source, which takes the per-pixel kernel."""
    import torch
    if dst == "down":
        (dh, dw), (sh, sw) = (5, 7), (9, 14)
    else:
        dh, dw = dst
        sh, sw = max(1, int(round(dh * pyr_scale))), max(1, int(round(dw * pyr_scale)))
        assert sh <= dh and sw <= dw
    rng = np.random.default_rng(dh * 1000 + dw)
    f = (rng.standard_normal((2, sh, sw, 2)) * 4).astype(np.float32)
    want = np.stack([oracle.resize_linear(f[i], dw, dh) * np.float32(1.0 / pyr_scale) for i in range(2)])
    for n in (1, 2):
        runs = []
        for poison in FLOAT_POISONS:
            src = _float_in(torch, torch_dev, f[:n], poison, row_dims=2)
            out, check = banded_out(torch, torch_dev, (n, dh, dw, 2), np.float32, row_dims=2)
            ctx.check(ctx._lib.nsof_stage_flow_upsample(ctx.ptr, n, src.data_ptr(), sw, sh, out.data_ptr(), dw, dh, pyr_scale))
            ctx.synchronize()
            runs.append((out.cpu().numpy(), check))
        _judge(f"flow_upsample {(sh, sw)} -> {(dh, dw)} scale {pyr_scale} n={n}", runs, want[:n])


@pytest.mark.parametrize("f32_mode", [0, 1], ids=["exact", "polyexp_f32"])
@pytest.mark.parametrize("poly_n,sigma", [(5, 1.2), (7, 1.5)])
def test_stage_polyexp(ctx, oracle, torch_dev, poly_n, sigma, f32_mode):
    """A workgroup owns SW = 256 - 2 * NP output columns (NP = poly_n rounded up to 4: 240 for both radii), a lane 4 of
    them, a step 4 rows: widths 1, 3, 5, SW - 1, SW, SW + 1, heights 1, 2, 5.  With NSOF_OPT_POLYEXP_F32 (k_polyexp, float
    sums: no oracle twin) only assertions (b) and (c) apply."""
    import torch
    from nsof import _lib
    np_ = (poly_n + 3) // 4 * 4
    sw = 256 - 2 * np_
    assert sw == 240
    ctx.set_option(_lib.OPT_POLYEXP_F32, f32_mode)
    try:
        for w in (1, 3, 5, sw - 1, sw, sw + 1):
            for h in (1, 2, 5):
                imgs = (np.random.default_rng(poly_n * 1000 + h * 300 + w).random((2, h, w)) * 255).astype(np.float32)
                want = None if f32_mode else np.stack([_rlayout(oracle.polyexp(imgs[i], poly_n, sigma)) for i in range(2)])
                for n in (1, 2):
                    runs = []
                    for poison in FLOAT_POISONS:
                        src = _float_in(torch, torch_dev, imgs[:n], poison)
                        out, check = banded_out(torch, torch_dev, (n, 5 * h * w), np.float32)
                        ctx.check(ctx._lib.nsof_stage_polyexp(ctx.ptr, n, src.data_ptr(), w, h, poly_n, sigma, out.data_ptr()))
                        ctx.synchronize()
                        runs.append((out.cpu().numpy(), check))
                    _judge(f"polyexp n={poly_n} {(h, w)} n_img={n} f32_mode={f32_mode}", runs, None if want is None else want[:n])
                    if f32_mode:   # every element was written with a number (the band pattern is a NaN)
                        assert np.isfinite(runs[0][0]).all(), (poly_n, (h, w), n)
    finally:
        ctx.set_option(_lib.OPT_POLYEXP_F32, 0)


def _pair_inputs(h, w):
    """R (2 pairs: [2][2][5hw] in the device layout), flow [2][h][w][2] and the oracle-layout pieces of two pairs."""
    st = [_stage_inputs(h * 100 + w + 11 * i, h, w) for i in range(2)]
    Rdev = np.stack([np.stack([_rlayout(R0), _rlayout(R1)]) for R0, R1, _ in st])
    flow = np.stack([fl for _, _, fl in st])
    return st, Rdev, flow


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (5, 67)], ids=["1x1", "3x5", "5x67"])
def test_stage_update_matrices(ctx, oracle, torch_dev, shape):
    import torch
    h, w = shape
    st, Rdev, flow = _pair_inputs(h, w)
    want = np.stack([_planar(oracle.update_matrices(*s)) for s in st])
    for n in (1, 2):
        runs = []
        for poison in FLOAT_POISONS:
            dR = _float_in(torch, torch_dev, Rdev[:n], poison)
            dF = _float_in(torch, torch_dev, flow[:n], poison, row_dims=2)
            out, check = banded_out(torch, torch_dev, (n, 5, h, w), np.float32)
            ctx.check(ctx._lib.nsof_stage_update_matrices(ctx.ptr, n, dR.data_ptr(), dF.data_ptr(), w, h, out.data_ptr()))
            ctx.synchronize()
            runs.append((out.cpu().numpy(), check))
        _judge(f"update_matrices {shape} n={n}", runs, want[:n])


def _iterate_case(ctx, oracle, torch_dev, h, w, winsize, exact, what):
    import torch
    st, Rdev, flow = _pair_inputs(h, w)
    want, tol = [], []
    for R0, R1, fl in st:
        M = oracle.update_matrices(R0, R1, fl)
        want.append(oracle.update_flow_blur(R0, R1, fl, M, winsize, False)[0])
        tol.append(F.blur_solve(M, winsize)[1])
    want, tol = np.stack(want), np.stack(tol)
    for n in (1, 2):
        runs = []
        for poison in FLOAT_POISONS:
            dR = _float_in(torch, torch_dev, Rdev[:n], poison)
            dF = _float_in(torch, torch_dev, flow[:n], poison, row_dims=2)
            out, check = banded_out(torch, torch_dev, (n, h, w, 2), np.float32, row_dims=2)
            ctx.check(ctx._lib.nsof_stage_iterate(ctx.ptr, n, dR.data_ptr(), dF.data_ptr(), w, h, winsize, out.data_ptr()))
            ctx.synchronize()
            runs.append((out.cpu().numpy(), check))
        _judge(f"iterate {what} {(h, w)} winsize {winsize} n={n}", runs, want[:n], None if exact else tol[:n])


@pytest.mark.parametrize("winsize", [3, 4, 15])
def test_stage_iterate_exact(ctx, oracle, torch_dev, winsize):
    """k_iterate_x (the default): strips of 192 columns, 4 rows per step: widths 2, 3, 5, 191, 192, 193, 197, heights 2, 3,
    5, 7.  The oracle's bits."""
    for w in (2, 3, 5, 191, 192, 193, 197):
        for h in (2, 3, 5, 7):
            _iterate_case(ctx, oracle, torch_dev, h, w, winsize, True, "k_iterate_x")


@pytest.mark.parametrize("row_bands,heights", [(0, (2, 5)), (4, (7, 9))], ids=["whole_strips", "row_bands4"])
@pytest.mark.parametrize("winsize", [3, 15])
def test_stage_iterate_fast_mode(ctx, oracle, torch_dev, winsize, row_bands, heights):
    """k_iterate_q (NSOF_OPT_EXACT_ROWSUMS = 0): strips of SW = (256 - 2m) & ~3 columns, 4 pixels per solve thread: widths
    SW - 1, SW, SW + 1, SW + 3; again cut into bands of 4 rows (NSOF_OPT_ROW_BANDS = 4) at heights 7 and 9.  This form
    sums each window directly and is not bit-exact: it is held to oracle.update_flow_blur within the bound
    farneback_f64.blur_solve derives; assertions (b) and (c) hold as everywhere."""
    from nsof import _lib
    m = winsize // 2
    sw = (256 - 2 * m) & ~3
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 0)
    try:
        ctx.set_option(_lib.OPT_ROW_BANDS, row_bands)
        for w in (sw - 1, sw, sw + 1, sw + 3):
            for h in heights:
                _iterate_case(ctx, oracle, torch_dev, h, w, winsize, False, f"k_iterate_q bands={row_bands}")
    finally:
        ctx.set_option(_lib.OPT_ROW_BANDS, 0)
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 1)


@pytest.mark.parametrize("shape", [(6, 64), (6, 194), (6, 198)], ids=["6x64", "6x194", "6x198"])
def test_stage_iterate_x_resample(ctx, oracle, torch_dev, shape):
    """k_iterate_xr on the smallest shape of tests/test_iterate_resample_gpu.py and on destinations of two strips.  The
    entry takes exact doublings only (width == 2 * src_w), so the two-strip widths are 194 and 198; the odd widths 193 and
    197 must be refused with NOTHING written -- neither the band nor the logical elements."""
    import torch
    from nsof import _lib
    h, w = shape
    winsize, ps = 5, 0.5
    st, Rdev, _ = _pair_inputs(h, w)
    rng = np.random.default_rng(w)
    coarse = (rng.standard_normal((2, h // 2, w // 2, 2)) * 1.5).astype(np.float32)
    want = []
    for i, (R0, R1, _) in enumerate(st):
        fine = oracle.resize_linear(coarse[i], w, h) * np.float32(1.0 / ps)
        want.append(oracle.update_flow_blur(R0, R1, fine, oracle.update_matrices(R0, R1, fine), winsize, False)[0])
    want = np.stack(want)
    for n in (1, 2):
        runs = []
        for poison in FLOAT_POISONS:
            dR = _float_in(torch, torch_dev, Rdev[:n], poison)
            dC = _float_in(torch, torch_dev, coarse[:n], poison, row_dims=2)
            out, check = banded_out(torch, torch_dev, (n, h, w, 2), np.float32, row_dims=2)
            ctx.check(ctx._lib.nsof_stage_iterate_x_resample(ctx.ptr, n, dR.data_ptr(), dC.data_ptr(), w // 2, h // 2, w, h,
                                                             winsize, ps, out.data_ptr()))
            ctx.synchronize()
            runs.append((out.cpu().numpy(), check))
        _judge(f"iterate_x_resample {shape} n={n}", runs, want[:n])
    if w > 190:   # the odd width next to it: refused, output untouched
        wo = w - 1
        dR = _float_in(torch, torch_dev, Rdev[:1, :, :5 * h * wo], QNAN)
        dC = _float_in(torch, torch_dev, coarse[:1], QNAN, row_dims=2)
        out, check = banded_out(torch, torch_dev, (1, h, wo, 2), np.float32, row_dims=2)
        rc = ctx._lib.nsof_stage_iterate_x_resample(ctx.ptr, 1, dR.data_ptr(), dC.data_ptr(), w // 2, h // 2, wo, h, winsize, ps,
                                                    out.data_ptr())
        assert rc == _lib.NSOF_EUNSUPPORTED
        ctx.synchronize()
        check()
        from guard_bands import PATTERN
        assert (_bits(out.cpu().numpy()) == PATTERN).all()


@pytest.mark.parametrize("winsize", [2, 15, 31])
@pytest.mark.parametrize("form", ["exact_pair", "fast", "gauss"])
def test_stage_blur_solve(ctx, oracle, torch_dev, form, winsize):
    """nsof_stage_blur_solve in both forms (k_blur_colsum + k_blur_rowsolve: the oracle's bits; k_blur_solve of the fast mode:
    within farneback_f64.blur_solve's bound of the oracle) and nsof_stage_gauss_blur_solve (farneback_gauss's bits)."""
    import torch
    from nsof import _lib
    entry = ctx._lib.nsof_stage_gauss_blur_solve if form == "gauss" else ctx._lib.nsof_stage_blur_solve
    ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 0 if form == "fast" else 1)
    try:
        for h, w in [(1, 1), (2, 3), (7, 65), (33, 47)]:
            st, _, _ = _pair_inputs(h, w)
            Ms = [oracle.update_matrices(*s) for s in st]
            if form == "gauss":
                want = np.stack([FG.gauss_blur_solve(M, winsize) for M in Ms])
            else:
                want = np.stack([oracle.update_flow_blur(*s, M, winsize, False)[0] for s, M in zip(st, Ms)])
            tol = np.stack([F.blur_solve(M, winsize)[1] for M in Ms]) if form == "fast" else None
            Mdev = np.stack([_planar(M) for M in Ms])
            for n in (1, 2):
                runs = []
                for poison in FLOAT_POISONS:
                    dM = _float_in(torch, torch_dev, Mdev[:n], poison)
                    out, check = banded_out(torch, torch_dev, (n, h, w, 2), np.float32, row_dims=2)
                    ctx.check(entry(ctx.ptr, n, dM.data_ptr(), w, h, winsize, out.data_ptr()))
                    ctx.synchronize()
                    runs.append((out.cpu().numpy(), check))
                _judge(f"blur_solve {form} {(h, w)} winsize {winsize} n={n}", runs, want[:n], None if tol is None else tol[:n])
    finally:
        ctx.set_option(_lib.OPT_EXACT_ROWSUMS, 1)


# ---- 3. whole calls ------------------------------------------------------------------------------------------------------
PARAMS = {"A": (0.5, 3, 15, 3, 5, 1.2, 0), "B": (0.6, 3, 3, 3, 10, 1.05, 0)}
CALL_SHAPES = [(7, 13), (33, 47), (61, 197)]
CALL_DTYPES = {"uint8": (0, 0x00, 0xFF), "uint16": (2, 0x0000, 0x8000)}
CALLS = [(s, p, d) for s in CALL_SHAPES for p in PARAMS for d in CALL_DTYPES]
CALL_IDS = [f"{s[0]}x{s[1]}-{p}-{d}" for s, p, d in CALLS]
_frames_cache, _flow_cache = {}, {}


def _call_frames(shape, dtype):
    """Four frames (4, h, w): smoothed noise that moves by (1, 2) pixels from frame to frame; 16-bit ones fill their range."""
    if (shape, dtype) not in _frames_cache:
        h, w = shape
        base = _noise_u8(h * 31 + w, 1, h + 8, w + 12)[0].astype(np.float32)
        base = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) / 4
        fr = np.stack([base[i:i + h, 2 * i:2 * i + w] for i in range(4)]).astype(np.uint8)
        fr = fr if dtype == "uint8" else fr.astype(np.uint16) * np.uint16(257)
        fr.setflags(write=False)
        _frames_cache[(shape, dtype)] = fr
    return _frames_cache[(shape, dtype)]


def _ref_flow(oracle, a, b, params):
    """The CPU reference of one pair: the oracle for 8-bit frames, farneback_f32 (the oracle's stages on float frames) for
    the others.  Computed once per pair and shared read-only."""
    key = (a.tobytes(), b.tobytes(), a.shape, a.dtype.name, params)
    if key not in _flow_cache:
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        flow = oracle.farneback(a, b, *params) if a.dtype == np.uint8 else \
            farneback_f32(oracle, a.astype(np.float32), b.astype(np.float32), *params)
        flow.setflags(write=False)
        _flow_cache[key] = flow
    return _flow_cache[key]


def _want_pairs(oracle, frames, n, params):
    return np.stack([_ref_flow(oracle, frames[i], frames[i + 1], params) for i in range(n)])


@pytest.mark.parametrize("shape,pname,dtype", CALLS, ids=CALL_IDS)
def test_lone_host_pair(ctx, oracle, shape, pname, dtype):
    """nsof_farneback_px: the flow goes into a host array with a padded flow_stride inside a banded host buffer; the frames
    are strided host views, one element past an aligned address, whose surroundings are poisoned."""
    import torch
    h, w = shape
    pt, poison_a, poison_b = CALL_DTYPES[dtype]
    fr = _call_frames(shape, dtype)
    want = _ref_flow(oracle, fr[0], fr[1], PARAMS[pname])
    runs = []
    for poison in (poison_a, poison_b):
        a, b = (surrounded_in(torch, "cpu", fr[i], fr.dtype.type(poison), pitch_extra=13, offset_elems=1) for i in (0, 1))
        out, check = banded_out(torch, "cpu", (h, w, 2), np.float32, pitch_extra=6, row_dims=2)
        ctx.check(ctx._lib.nsof_farneback_px(ctx.ptr, pt, a.data_ptr(), a.row_stride, b.data_ptr(), b.row_stride, w, h,
                                             out.data_ptr(), out.row_stride, *PARAMS[pname]))
        runs.append((out.numpy().copy(), check))
    _judge(f"lone host pair {shape} {pname} {dtype}", runs, want)


@pytest.mark.parametrize("shape,pname,dtype", CALLS, ids=CALL_IDS)
def test_device_batch(ctx, oracle, torch_dev, shape, pname, dtype):
    """nsof_farneback_px_batch_dev with 1 and 3 pairs, in the default small-batch form (k_lat_*) and with
    NSOF_OPT_SMALL_BATCH_JOBS = 0 (k_iterate_x); frames with ragged pitch and pair padding, the dense flows in bands."""
    import torch
    from nsof import _lib
    h, w = shape
    pt, poison_a, poison_b = CALL_DTYPES[dtype]
    fr = _call_frames(shape, dtype)
    want = _want_pairs(oracle, fr, 3, PARAMS[pname])
    try:
        for jobs in (64, 0):
            ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, jobs)
            for n in (1, 3):
                runs = []
                for poison in (poison_a, poison_b):
                    lay = dict(pitch_extra=5, item_extra=3, offset_elems=1)
                    dp = surrounded_in(torch, torch_dev, fr[:n], fr.dtype.type(poison), **lay)
                    dn = surrounded_in(torch, torch_dev, fr[1:n + 1], fr.dtype.type(poison), **lay)
                    out, check = banded_out(torch, torch_dev, (n, h, w, 2), np.float32, row_dims=2)
                    ctx.check(ctx._lib.nsof_farneback_px_batch_dev(ctx.ptr, pt, n, dp.data_ptr(), dn.data_ptr(), dp.row_stride,
                                                                   dp.item_stride, w, h, out.data_ptr(), *PARAMS[pname]))
                    ctx.synchronize()
                    runs.append((out.cpu().numpy(), check))
                _judge(f"device batch {shape} {pname} {dtype} n={n} small_batch_jobs={jobs}", runs, want[:n])
    finally:
        ctx.set_option(_lib.OPT_SMALL_BATCH_JOBS, 64)


@pytest.mark.parametrize("shape,pname,dtype", CALLS, ids=CALL_IDS)
def test_device_sequence(ctx, oracle, torch_dev, shape, pname, dtype):
    """nsof_farneback_px_sequence_dev over 2 and 4 frames (rows and frames aligned for the vector forms this time)."""
    import torch
    h, w = shape
    pt, poison_a, poison_b = CALL_DTYPES[dtype]
    fr = _call_frames(shape, dtype)
    want = _want_pairs(oracle, fr, 3, PARAMS[pname])
    for n_frames in (2, 4):
        runs = []
        for poison in (poison_a, poison_b):
            d = surrounded_in(torch, torch_dev, fr[:n_frames], fr.dtype.type(poison), pitch_extra=16 + (-w) % 16, item_extra=32)
            out, check = banded_out(torch, torch_dev, (n_frames - 1, h, w, 2), np.float32, row_dims=2)
            ctx.check(ctx._lib.nsof_farneback_px_sequence_dev(ctx.ptr, pt, n_frames, d.data_ptr(), d.row_stride, d.item_stride, w, h,
                                                              out.data_ptr(), *PARAMS[pname]))
            ctx.synchronize()
            runs.append((out.cpu().numpy(), check))
        _judge(f"device sequence {shape} {pname} {dtype} n_frames={n_frames}", runs, want[:n_frames - 1])


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("dtype", list(CALL_DTYPES))
def test_device_pair_list(ctx, oracle, torch_dev, pname, dtype):
    """nsof_farneback_px_batch_desc_dev on a list of the three shapes: the items' crops are cut from one poisoned canvas
    per side, each item's flow has its own padded flow_stride, all three in one banded buffer."""
    import torch
    from nsof import _lib
    from guard_bands import banded_items
    pt, poison_a, poison_b = CALL_DTYPES[dtype]
    at = {(7, 13): (2, 3), (33, 47): (12, 5), (61, 197): (15, 70)}   # (y, x) of each item in the 80 x 280 canvas
    frames = {s: _call_frames(s, dtype) for s in CALL_SHAPES}
    want = [_ref_flow(oracle, frames[s][0], frames[s][1], PARAMS[pname]) for s in CALL_SHAPES]
    runs = []
    for poison in (poison_a, poison_b):
        canvases = []
        for side in (0, 1):
            cv = np.full((80, 280), poison, frames[CALL_SHAPES[0]].dtype)
            for s, (y, x) in at.items():
                cv[y:y + s[0], x:x + s[1]] = frames[s][side]
            canvases.append(surrounded_in(torch, torch_dev, cv, cv.dtype.type(poison), pitch_extra=3, offset_elems=1))
        outs, check = banded_items(torch, torch_dev, [s + (2,) for s in CALL_SHAPES], np.float32, pitch_extra=6, row_dims=2)
        descs = (_lib.PairDesc * 3)()
        es = canvases[0].element_size()
        for k, s in enumerate(CALL_SHAPES):
            y, x = at[s]
            off = (y * (canvases[0].row_stride // es) + x) * es
            descs[k] = _lib.PairDesc(canvases[0].data_ptr() + off, canvases[0].row_stride, canvases[1].data_ptr() + off,
                                     canvases[1].row_stride, s[1], s[0], outs[k].data_ptr(), outs[k].row_stride)
        ctx.check(ctx._lib.nsof_farneback_px_batch_desc_dev(ctx.ptr, pt, 3, descs, *PARAMS[pname]))
        ctx.synchronize()
        runs.append(([o.cpu().numpy() for o in outs], check))
    for k, s in enumerate(CALL_SHAPES):   # the band check belongs to the whole buffer: raised with the first item
        _judge(f"device pair list {pname} {dtype} item {k} {s}", [(r[0][k], r[1] if k == 0 else (lambda: None)) for r in runs],
               want[k])


def test_gated_roi_sequence(ctx, oracle, torch_dev):
    """nsof_farneback_px_roi_sequence_dev, 3 frames of 61 x 197 with two rectangles per frame: inside the rectangles the
    crops' reference flows, outside them zeros (the entry zero-fills the canvases), and clean bands."""
    import torch
    H, W = 61, 197
    params = PARAMS["B"]
    fr = _call_frames((H, W), "uint8")[:3]
    table = [(5, 3, 52, 40), (100, 20, 197, 61)]   # x0, y0, x1, y1
    rects = np.zeros((3, 2, 4), np.int32)
    rects[:] = table
    counts = np.full(3, 2, np.int32)
    want = np.zeros((2, H, W, 2), np.float32)
    for k in range(2):
        for x0, y0, x1, y1 in table:
            want[k, y0:y1, x0:x1] = _ref_flow(oracle, fr[k, y0:y1, x0:x1], fr[k + 1, y0:y1, x0:x1], params)
    d_counts, d_rects = torch.from_numpy(counts).to(torch_dev), torch.from_numpy(rects).to(torch_dev)
    runs = []
    for poison in (0x00, 0xFF):
        d = surrounded_in(torch, torch_dev, fr, np.uint8(poison), pitch_extra=5, item_extra=3, offset_elems=1)
        out, check = banded_out(torch, torch_dev, (2, H, W, 2), np.float32, row_dims=2)
        calls, pixels = C.c_longlong(), C.c_longlong()
        ctx.check(ctx._lib.nsof_farneback_px_roi_sequence_dev(ctx.ptr, 0, 3, d.data_ptr(), d.row_stride, d.item_stride, W, H,
                                                              d_counts.data_ptr(), d_rects.data_ptr(), 2, out.data_ptr(), *params,
                                                              0, C.byref(calls), C.byref(pixels)))
        ctx.synchronize()
        assert calls.value == 4
        runs.append((out.cpu().numpy(), check))
    _judge("gated ROI sequence", runs, want)
