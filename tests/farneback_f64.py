"""A float64 reference of the Farneback stages, written from the algorithm's definition (test-only).

The oracle (oracle/farneback_ref.c) and the HIP kernels restate the same float32 operation order and were written to
agree with each other, so a mistake made in both is invisible to the bit-exact tests.  This module states every stage
once more, in NumPy float64, from what the stage *is* rather than how cv2 orders its arithmetic:

* ``gaussian_blur``  separable Gaussian (getGaussianKernel taps, unrounded), BORDER_REFLECT_101 on both axes;
* ``resize_linear``  INTER_LINEAR: source coordinate (d + 0.5) * (1 / (dsize / ssize)) - 0.5 in double, columns
  clamped to the last one (weight zeroed), rows clamped by index (weights kept);
* ``pyr_level``      level k of the pyramid: the blur of the full frame, then the resize;
* ``polyexp``        the Gaussian-weighted least-squares fit of 1, x, y, x^2, y^2, xy over (2n+1)^2 pixels with
  replicated borders in both directions, solved with the full 6x6 moment matrix (the cv2 kernel uses four
  constants of its inverse instead);
* ``update_matrices`` the bilinear sample of R1 at the float32 position (x + dx, y + dy), the out-of-image branch and
  the five-pixel border weights {.14, .14, .4472, .4472, .4472};
* ``blur_solve``     a (2m+1)^2 box filter (m = winsize // 2, replicated borders, normalised by 1 / winsize^2), then the
  2x2 solve with 1e-3 added to the determinant;
* ``flow_upsample``  ``resize_linear`` of the flow times 1 / pyr_scale.

Every stage returns ``(value, tol)``: the float64 result and a per-element bound on how far a float32 implementation of
the same stage, fed the same float32 inputs, may lie from it.  The bounds are forward-error bounds of the float32
arithmetic, not fitted figures (u = 2^-24, the unit roundoff of float32; ``E`` the same stage evaluated on absolute
values with absolute weights, i.e. the sum of the magnitudes of every term; every rounding may also underflow, which
costs at most 2^-149 absolute more, and each bound below carries that term once per rounding it counts):

* blur           tol = (2 ksize + 6) u E: one rounding per tap (ksize taps) and per partial sum, two passes, plus
                 the rounding of each tap to float32;
* resize         tol = 8 u E + 2 u (max(sw, sh) + 2) max|src|: the blends round 6 times; the source coordinate is
                 rounded to float32 once (|df| <= u |f|), which moves the sample by at most |df| times the local
                 difference <= 2 max|src|;
* polyexp        tol = (4 n + 24) u E + 4 u E_inv: the vertical pass sums 2n + 1 float32 products (rounded) per
                 moment, the taps and the products with x, x^2 are rounded to float32; the horizontal pass and the
                 final combination are in double.  E is the fit evaluated with |invG| on the moments of |I| with
                 |x^a y^b| weights, so the bound covers the cancellation of channels 2 and 3.  The moment matrix is
                 built from the rounded taps (|dG| <= 4 u |G|, which also covers the four-constant form cv2 uses in
                 place of the full inverse) and d(invG) = -invG dG invG to first order, so E_inv is the same fit with
                 |invG| |G| |invG| in place of |invG|: the term that grows with the matrix's condition number (large
                 for n = 1 at sigma 0.3);
* update_matrices tol = 16 u E: at most 4 roundings in the sample, 3 in r2..r6, 3 in each product of M;
* blur_solve     the column sums add float32 differences M[y+m] - M[y-m-1] (error <= u |difference| <= 2 u max|M|)
                 once per row, so each box mean is off by at most d = (2m+1) (h + 2m + 2) 2 u max|M_c| / winsize^2
                 (double sums add nothing at this scale); to first order the solve turns that into
                 (d_num + |flow| d_det) / det, with d_num, d_det the sums of |partial derivatives| times d, doubled,
                 plus 2 u |flow| for the final rounding to float32;
* flow_upsample  the resize bound, times 1 / pyr_scale, plus 2 u |value| for the float32 scale factor.

The measured errors of the oracle and of the device stay inside these bounds (at most 0.4 of a bound on the shapes of
tests/test_farneback_f64.py); the bounds are not tuned to them.  Non-finite values are outside this module: the tests
that feed them compare the device with the oracle bit for bit instead."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149   # the smallest float32 subnormal: the absolute error of a rounding that underflows
FLT_EPSILON = 1.1920928955078125e-07
BORDER_WEIGHTS = (0.14, 0.14, 0.4472, 0.4472, 0.4472)   # from the outermost pixel inwards


# ---------------------------------------------------------------- pyramid
def reflect101(i, n):
    """BORDER_REFLECT_101 index (... 2 1 | 0 1 2 ... n-1 | n-2 ...), any distance outside, n == 1 included."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def gaussian_taps(ksize, sigma):
    """getGaussianKernel(ksize, sigma) in float64, for the two forms the pyramid uses: sigma > 0 (levels >= 1), the
    normalised Gaussian; sigma = 0 (level 0, ksize 3), cv2's fixed table [1/4, 1/2, 1/4]."""
    if sigma <= 0:
        if ksize != 3:
            raise ValueError("the pyramid blurs with sigma <= 0 only at ksize 3")
        return np.array([0.25, 0.5, 0.25])
    x = np.arange(ksize) - (ksize - 1) / 2
    t = np.exp(-x * x / (2.0 * sigma * sigma))
    return t / t.sum()


def _sep_filter(a, taps, idx_rows, idx_cols):
    """sum_j taps[j] a[idx_rows[y + j], :] then the same over columns (a: h x w float64)."""
    h, w = a.shape
    k = len(taps)
    t = sum(taps[j] * a[:, idx_cols[j:j + w]] for j in range(k))
    return sum(taps[j] * t[idx_rows[j:j + h], :] for j in range(k))


def gaussian_blur(src, ksize, sigma):
    src = np.asarray(src, np.float64)
    h, w = src.shape
    if ksize == 1:
        return src.copy(), np.zeros_like(src)
    taps = gaussian_taps(ksize, sigma)
    r = ksize // 2
    rows, cols = reflect101(np.arange(-r, h + r), h), reflect101(np.arange(-r, w + r), w)
    val = _sep_filter(src, taps, rows, cols)
    env = _sep_filter(np.abs(src), taps, rows, cols)
    return val, (2 * ksize + 6) * (U * env + TINY)


def _linear_coords(dsize, ssize):
    scale = 1.0 / (dsize / ssize)
    f = (np.arange(dsize) + 0.5) * scale - 0.5
    s = np.floor(f).astype(np.int64)
    return s, f - s, np.abs(f)


def resize_linear(src, dw, dh):
    """INTER_LINEAR resize of an h x w or h x w x c array; returns (value, tol)."""
    src = np.asarray(src, np.float64)
    sh, sw = src.shape[:2]
    if (sw, sh) == (dw, dh):
        return src.copy(), np.zeros_like(src)
    a3 = src.reshape(sh, sw, -1)
    sx, ax, _ = _linear_coords(dw, sw)
    low, high = sx < 0, sx >= sw - 1
    ax = np.where(low | high, 0.0, ax)
    sx = np.where(low, 0, np.where(high, sw - 1, sx))
    sx1 = np.minimum(sx + 1, sw - 1)
    sy, ay, _ = _linear_coords(dh, sh)
    sy0, sy1 = np.clip(sy, 0, sh - 1), np.clip(sy + 1, 0, sh - 1)

    def blend(v):
        hrow = v[:, sx, :] * (1 - ax)[None, :, None] + v[:, sx1, :] * ax[None, :, None]
        return hrow[sy0] * (1 - ay)[:, None, None] + hrow[sy1] * ay[:, None, None]

    val = blend(a3)
    mag = np.abs(a3).max() if a3.size else 0.0
    tol = 8 * (U * blend(np.abs(a3)) + TINY) + 2 * U * (max(sw, sh) + 2) * mag
    shape = (dh, dw) + src.shape[2:]
    return val.reshape(shape), tol.reshape(shape)


def level_geometry(w, h, pyr_scale, k):
    """(wk, hk, ksize, sigma) of level k: scale = pyr_scale^k (k products), sigma = (1/scale - 1) / 2,
    ksize = max(3, round(5 sigma) | 1), sizes round(w scale), round(h scale); rounding half to even."""
    scale = 1.0
    for _ in range(k):
        scale *= pyr_scale
    sigma = (1.0 / scale - 1) * 0.5
    ksize = max(3, int(round(sigma * 5)) | 1)
    return int(round(w * scale)), int(round(h * scale)), ksize, sigma


def pyr_level(img, pyr_scale, k):
    img = np.asarray(img, np.float64)
    h, w = img.shape
    wk, hk, ksize, sigma = level_geometry(w, h, pyr_scale, k)
    b, tb = gaussian_blur(img, ksize, sigma)
    val, tr = resize_linear(b, wk, hk)
    carried, _ = resize_linear(tb, wk, hk)   # the blur's error passes through the blend's convex weights
    return val, tr + carried


# ---------------------------------------------------------------- polynomial expansion
def poly_basis(n, sigma):
    """Taps g (float64, unrounded), and the 6x6 moment matrix G of the basis (1, x, y, x^2, y^2, xy) under the weights
    g(x) g(y) over [-n, n]^2.  sigma < FLT_EPSILON selects sigma = 0.3 n (FarnebackPrepareGaussian)."""
    if sigma < FLT_EPSILON:
        sigma = n * 0.3
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * sigma * sigma))
    g /= g.sum()
    yy, xx = np.meshgrid(x, x, indexing="ij")
    basis = np.stack([np.ones_like(xx), xx, yy, xx * xx, yy * yy, xx * yy]).reshape(6, -1)
    wgt = np.outer(g, g).ravel()
    G = (basis * wgt) @ basis.T
    return g, x, G


def _moments(img, g, x, n, absolute):
    """The six weighted moments sum g(u) g(v) b_i(u, v) I(y + v, x + u) with replicated borders; absolute=True uses
    |I| and |b_i| (the magnitude envelope)."""
    P = np.pad(np.asarray(img, np.float64), n, mode="edge")
    if absolute:
        P, x = np.abs(P), np.abs(x)
    h, w = img.shape
    k = 2 * n + 1
    # vertical moments v_a = sum_v g(v) v^a P[y + v]   (a = 0, 1, 2), then horizontal moments of each
    v = [sum(g[j] * x[j] ** a * P[j:j + h, :] for j in range(k)) for a in range(3)]

    def hm(arr, b):
        return sum(g[j] * x[j] ** b * arr[:, j:j + w] for j in range(k))

    # order of the basis: 1, x, y, x^2, y^2, xy
    return np.stack([hm(v[0], 0), hm(v[0], 1), hm(v[1], 0), hm(v[0], 2), hm(v[2], 0), hm(v[1], 1)], axis=-1)


def polyexp(img, n, sigma):
    """R (h x w x 5) in cv2's channel order: (c_y, c_x, c_yy, c_xx, c_xy) of the local fit
    I(x + u, y + v) ~ c_1 + c_x u + c_y v + c_xx u^2 + c_yy v^2 + c_xy u v."""
    g, x, G = poly_basis(n, sigma)
    invG = np.linalg.inv(G)
    c = _moments(img, g, x, n, False) @ invG.T
    m_abs = _moments(img, g, x, n, True)
    e = m_abs @ np.abs(invG).T
    cond = np.abs(invG) @ np.abs(G) @ np.abs(invG)   # first-order growth of an error in G through its inverse
    e_inv = m_abs @ cond.T
    order = [2, 1, 4, 3, 5]
    return c[..., order], (4 * n + 24) * (U * e[..., order] + TINY) + 4 * U * e_inv[..., order]


# ---------------------------------------------------------------- matrix update
def border_scale(w, h):
    """Per-pixel product of the border weights of the column and of the row (1 away from the 5-pixel border)."""
    def axis(n):
        s = np.ones(n)
        for i, b in enumerate(BORDER_WEIGHTS):
            if i < n:
                s[i] *= b
                s[n - 1 - i] *= b
        return s
    return np.outer(axis(h), axis(w))


def update_matrices(R0, R1, flow):
    """M (h x w x 5: G11, G12, G22, h1, h2) from the two expansions and the flow.  The sample position is the float32
    sum x + dx (the flow is float32); the sample itself and everything after it are float64."""
    R0 = np.asarray(R0, np.float64)
    R1 = np.asarray(R1, np.float64)
    flow = np.asarray(flow, np.float32)
    h, w = flow.shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    fx = (xx.astype(np.float32) + flow[..., 0]).astype(np.float64)
    fy = (yy.astype(np.float32) + flow[..., 1]).astype(np.float64)
    x1, y1 = np.floor(fx), np.floor(fy)
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    ax, ay = fx - x1, fy - y1
    xi = np.where(inside, x1, 0).astype(np.int64)
    yi = np.where(inside, y1, 0).astype(np.int64)
    xj, yj = np.minimum(xi + 1, w - 1), np.minimum(yi + 1, h - 1)
    a00, a01 = ((1 - ax) * (1 - ay))[..., None], (ax * (1 - ay))[..., None]
    a10, a11 = ((1 - ax) * ay)[..., None], (ax * ay)[..., None]
    dx, dy = flow[..., 0].astype(np.float64), flow[..., 1].astype(np.float64)
    scale = border_scale(w, h)

    def terms(R0, R1, absolute):
        s = a00 * R1[yi, xi] + a01 * R1[yi, xj] + a10 * R1[yj, xi] + a11 * R1[yj, xj]
        s = np.where(inside[..., None], s, 0.0)
        sign = 1.0 if absolute else -1.0
        half = np.where(inside, 0.5, 1.0)    # inside: the mean of R0 and the sample; outside: R0 alone
        r2 = (R0[..., 0] + sign * s[..., 0]) * 0.5
        r3 = (R0[..., 1] + sign * s[..., 1]) * 0.5
        r4 = (R0[..., 2] + s[..., 2]) * half
        r5 = (R0[..., 3] + s[..., 3]) * half
        r6 = (R0[..., 4] + s[..., 4]) * half * 0.5
        ddx, ddy = (np.abs(dx), np.abs(dy)) if absolute else (dx, dy)
        r2 = r2 + r4 * ddy + r6 * ddx
        r3 = r3 + r6 * ddy + r5 * ddx
        r2, r3, r4, r5, r6 = (r * scale for r in (r2, r3, r4, r5, r6))
        if absolute:
            r2, r3, r4, r5, r6 = (np.abs(r) for r in (r2, r3, r4, r5, r6))
        return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3],
                        axis=-1)

    val = terms(R0, R1, False)
    env = terms(np.abs(R0), np.abs(R1), True)
    return val, 16 * (U * env + TINY)


# ---------------------------------------------------------------- blur + solve
def box_mean(M, winsize):
    """Mean over the (2m+1)^2 window, m = winsize // 2, replicated borders, divided by winsize^2 (cv2's scale, which
    for an even winsize is not the window's own area)."""
    M = np.asarray(M, np.float64)
    h, w = M.shape[:2]
    m = winsize // 2
    P = np.pad(M, ((m, m), (m, m), (0, 0)), mode="edge")
    c = np.cumsum(np.cumsum(np.pad(P, ((1, 0), (1, 0), (0, 0))), axis=0), axis=1)
    k = 2 * m + 1
    s = c[k:k + h, k:k + w] - c[0:h, k:k + w] - c[k:k + h, 0:w] + c[0:h, 0:w]
    return s / (winsize * winsize)


def blur_solve(M, winsize):
    """flow (h x w x 2) from M; returns (value, tol)."""
    M = np.asarray(M, np.float64)
    h = M.shape[0]
    m = winsize // 2
    b = box_mean(M, winsize)
    g11, g12, g22, h1, h2 = (b[..., i] for i in range(5))
    det = g11 * g22 - g12 * g12 + 1e-3
    fx = (g11 * h2 - g12 * h1) / det
    fy = (g22 * h1 - g12 * h2) / det
    d = (2 * m + 1) * (h + 2 * m + 2) * 2 * U * np.abs(M).reshape(-1, 5).max(axis=0) / (winsize * winsize)
    d11, d12, d22, dh1, dh2 = d
    ddet = np.abs(g22) * d11 + np.abs(g11) * d22 + 2 * np.abs(g12) * d12
    dnx = np.abs(h2) * d11 + np.abs(g11) * dh2 + np.abs(h1) * d12 + np.abs(g12) * dh1
    dny = np.abs(h1) * d22 + np.abs(g22) * dh1 + np.abs(h2) * d12 + np.abs(g12) * dh2
    ad = np.abs(det)
    tx = 2 * (dnx + np.abs(fx) * ddet) / ad + 2 * (U * np.abs(fx) + TINY)
    ty = 2 * (dny + np.abs(fy) * ddet) / ad + 2 * (U * np.abs(fy) + TINY)
    return np.stack([fx, fy], axis=-1), np.stack([tx, ty], axis=-1)


def flow_upsample(flow, dw, dh, pyr_scale):
    v, t = resize_linear(flow, dw, dh)
    a = 1.0 / pyr_scale
    return v * a, t * a + 2 * (U * np.abs(v * a) + TINY)


def within(got, ref, tol):
    """(ok, worst fraction of the bound used): got is float32, ref/tol float64, all finite."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    frac = err / np.maximum(tol, 1e-300)
    frac = np.where(err == 0, 0.0, frac)
    worst = float(frac.max()) if frac.size else 0.0
    return bool(np.isfinite(got).all() and worst <= 1.0), worst
