"""Hand-made flow fields for the heads that consume a flow on the device (colour coding, prediction warp, motion mask)
with the values a float-frame Farneback flow can hold: NaN, +-inf, finite values whose square overflows float32, a
subnormal, -0.0 -- in u only, in v only and in both, at the frame's corners, on its edges and inside.  Shared by
tests/test_heads_nonfinite_cpu.py (what the CPU references make of them) and tests/test_heads_nonfinite_gpu.py (the
kernels against those references).  Everything here is host NumPy; nothing touches a device.
"""
import functools

import numpy as np

NAN, INF = np.nan, np.inf
SINGLES = (NAN, INF, -INF, 3e38, -3e38, 2.0 ** 64, -2.0 ** 64, 1e-40, -0.0)
PAIRS = ((INF, NAN), (INF, -INF))
FINITE_DIVISOR = (NAN, 1e-40, -0.0)                    # the largest magnitude stays finite: ordinary colours remain
INFINITE_DIVISOR = (INF, -INF, 3e38, -3e38, 2.0 ** 64, -2.0 ** 64, NAN)
WARP_EXTRA = (1e10, -1e10)                             # finite, but x32 leaves the int range

H, W = 24, 70                                          # the colour and warp fields: two 64-px groups, the second partial
MASK_H, MASK_W = 37, 70
FARNEBACK_ARGS = (0.5, 3, 15, 3, 5, 1.2, 0)            # parameter set A
COLOUR_SHAPES = ((1, 1), (5, 3), (16, 256), (17, 257), (33, 255), (4, 1025))


def vectors(singles, pairs=()):
    """Every single in u only, in v only and in both (None = the field's own value), every pair both ways round."""
    out = []
    for s in singles:
        out += [(s, None), (None, s), (s, s)]
    for a, b in pairs:
        out += [(a, b), (b, a)]
    return out


def spots(h, w, n, rng):
    """n distinct pixels: the four corners, four edge pixels, then interior ones."""
    first = [(0, 0), (h - 1, w - 1), (0, w - 1), (h - 1, 0), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1)]
    interior = [(y, x) for y in range(1, h - 1) for x in range(1, w - 1)]
    pick = first + [interior[i] for i in rng.permutation(len(interior))[:max(0, n - len(first))]]
    assert len(set(pick)) == len(pick) >= n
    return pick[:n]


def special_flow(h, w, seed, singles, pairs=(), scale=1.5):
    """Gaussian flow of the given scale with the special vectors at spots(), in an order drawn from the seed (so which
    special meets a corner differs from field to field) -> (float32 [h][w][2], the pixels changed)."""
    rng = np.random.default_rng(seed)
    flow = (rng.standard_normal((h, w, 2)) * scale).astype(np.float32)
    vecs = vectors(singles, pairs)
    vecs = [vecs[i] for i in rng.permutation(len(vecs))]
    where = spots(h, w, len(vecs), rng)
    for (y, x), (u, v) in zip(where, vecs):
        if u is not None:
            flow[y, x, 0] = u
        if v is not None:
            flow[y, x, 1] = v
    return flow, where


@functools.lru_cache(maxsize=None)
def _colour_fields():
    nan_f, _ = special_flow(H, W, 101, FINITE_DIVISOR, scale=2.0)
    inf_f, _ = special_flow(H, W, 102, INFINITE_DIVISOR, PAIRS, scale=2.0)
    fin_f = (np.random.default_rng(103).standard_normal((H, W, 2)) * 2.0).astype(np.float32)
    return nan_f, inf_f, fin_f


def colour_fields():
    """{"nan": NaNs (and the harmless finite specials) only, "inf": infinities and overflowing finites, "finite"}."""
    return {k: v.copy() for k, v in zip(("nan", "inf", "finite"), _colour_fields())}


def shape_field(h, w):
    """Gaussian flow with a NaN in the last column and in the last row (for (1, 1): the one pixel)."""
    flow = (np.random.default_rng(h * 10007 + w).standard_normal((h, w, 2)) * 2.0).astype(np.float32)
    flow[h - 1, w - 1, 0] = NAN
    if h > 1:
        flow[h - 1, 0] = NAN
        flow[0, w - 1, 1] = NAN
    if w > 2:
        flow[h - 1, w // 2, 1] = NAN
    return flow


def warp_flow(seed):
    """H x W flow of +-1.5 px with every special, +-1e10 included."""
    return special_flow(H, W, seed, SINGLES + WARP_EXTRA, PAIRS, scale=1.5)[0]


WARP_RECTS = ((0, 0, W, H), (9, 5, 58, 19), (W - 1, H - 1, W, H))


def remap_maps(sw, sh, bad, default=(2.25, 3.5)):
    """Maps [3 + 5][len(bad)] as tests/test_nonfinite_cpu.py lays them out: row 0 the bad values in x, row 1 in y, row 2
    in both, the other axis at its default; then five rows of taps around the source's right and left edge (x = w-3,
    w-2, w-1 with and without a fraction, -0.5) at rows above, inside and below the source."""
    n = len(bad)
    taps_x = [sw - 3 + 0.25, sw - 2 + 0.25, sw - 1 + 0.25, -0.5, sw - 3.0, sw - 2.0, sw - 1.0, sw - 2.5, 0.5 / 32]
    taps_y = [-0.5, 0.0, 0.25, sh - 2 + 0.5, sh - 1 + 0.25]
    mx = np.full((3 + len(taps_y), n), default[0], np.float32)
    my = np.full((3 + len(taps_y), n), default[1], np.float32)
    for j, v in enumerate(bad):
        mx[0, j] = v
        my[1, j] = v
        mx[2, j] = my[2, j] = v
    for i, ty in enumerate(taps_y):
        mx[3 + i] = [taps_x[j % len(taps_x)] for j in range(n)]
        my[3 + i] = ty
    return mx, my


REMAP_SOURCES_3CH = ((1, 1), (1, 2), (2, 1), (2, 3), (3, 2))     # h x w: narrower than the 8-byte two-tap load


def region_of(rects, h, w, merge_padding=None):
    """The pixels predict_sequence_dev warps for a table row: the union of its rectangles, or their bounding box
    padded by merge_padding and clipped to the frame."""
    m = np.zeros((h, w), bool)
    if not len(rects):
        return m
    if merge_padding is None:
        for x0, y0, x1, y1 in rects:
            m[y0:y1, x0:x1] = True
        return m
    r = np.asarray(rects)
    x0, y0 = max(0, r[:, 0].min() - merge_padding), max(0, r[:, 1].min() - merge_padding)
    x1, y1 = min(w, r[:, 2].max() + merge_padding), min(h, r[:, 3].max() + merge_padding)
    m[y0:y1, x0:x1] = True
    return m


# the table of the sequence warp: map 0 two overlapping rectangles, map 1 none, map 2 one that touches the frame's edge.
# Slots past a row's count hold the whole frame: a kernel that read them would warp everything.
SEQ_COUNTS = (2, 0, 1)
SEQ_RECTS = (((6, 3, 40, 15), (30, 10, 66, 22), (0, 0, W, H)),
             ((0, 0, W, H), (0, 0, W, H), (0, 0, W, H)),
             ((50, 12, W, H), (0, 0, W, H), (0, 0, W, H)))


# (u, v) float32 pairs around the threshold 1: name -> (vector, moves).  (0.6, 0.8) as float32 has the float64 magnitude
# 1 + 2.4e-8 (moves) and the float32 magnitude 1 exactly (would not); so have the two after it.
MASK_MARKS = {"one": ((1.0, 0.0), False), "one_v": ((0.0, -1.0), False), "six_eight": ((0.6, 0.8), True),
              "f32_rounds_down_a": ((0.5398502945899963, 0.84176105260849), True),
              "f32_rounds_down_b": ((0.9115411043167114, 0.41120898723602295), True),
              "just_above": ((float(np.nextafter(np.float32(1), np.float32(2))), 0.0), True),
              "lone_a": ((3.0, 0.0), True), "lone_b": ((0.0, -7.5), True), "lone_c": ((2.0, 2.0), True)}


@functools.lru_cache(maxsize=None)
def _mask_flows():
    out = []
    for seed in (201, 202):
        flow, used = special_flow(MASK_H, MASK_W, seed, SINGLES, PAIRS, scale=0.3)
        flow[20:29, 40:52] += np.float32(2.0)                     # a moving block the closing keeps
        used = set(used)
        free = [(y, x) for y in range(3, MASK_H - 3, 4) for x in range(5, 36, 6)
                if not any((y + j, x + i) in used for j in (-1, 0, 1) for i in (-1, 0, 1))]
        marks = {}
        for (name, (vec, _)), (y, x) in zip(MASK_MARKS.items(), free):
            if name.startswith("lone"):                          # isolated: nothing around it moves
                flow[y - 1:y + 2, x - 1:x + 2] = np.float32(0.125)
            flow[y, x] = vec
            marks[name] = (y, x)
        assert len(marks) == len(MASK_MARKS)
        out.append((flow, marks))
    return out


def mask_flows():
    """Two MASK_H x MASK_W fields of +-0.3 px (below the threshold) with every special, a moving block, and the marks of
    MASK_MARKS at free pixels -> [(flow, {mark: (y, x)})]."""
    return [(f.copy(), dict(m)) for f, m in _mask_flows()]


MASK_CHAINS = ((0, 10), (1, 3), (5, 10))                         # (iterations, ksize)
MASK_BOXES = (((5, 4, 50, 30), (40, 20, MASK_W, MASK_H)), ((0, 0, MASK_W, MASK_H), (0, 22, 38, MASK_H)))


@functools.lru_cache(maxsize=None)
def farneback_nan_case(oracle):
    """Part 3: float32 frames scaled to 4e20, where the oracle's Farneback flow is NaN on most pixels and finite on the
    rest -> (prev, next, the oracle's flow)."""
    from test_float_reference import farneback_f32, shifted_pair
    prev, nxt = shifted_pair(3, 64, 96, 0.0, 4e20)
    prev, nxt = prev.astype(np.float32), nxt.astype(np.float32)
    flow = farneback_f32(oracle, prev, nxt, *FARNEBACK_ARGS)
    flow.setflags(write=False)
    return prev, nxt, flow


def float64_mask(flow, thresh=1.0):
    """The threshold alone, from its definition in NumPy float64 (a NaN magnitude compares false)."""
    with np.errstate(invalid="ignore", over="ignore"):
        u, v = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
        return np.where(np.sqrt(u * u + v * v) > thresh, np.uint8(255), np.uint8(0))
