"""NumPy float32 restatement of the Gaussian window of Farneback's iteration (OPTFLOW_FARNEBACK_GAUSSIAN = 256):
FarnebackUpdateFlow_GaussianBlur, and the whole call composed from the oracle's stage functions.

A helper, not a test module.  With m = winsize // 2 and sigma = 0.3 m, in upstream's order:

  taps        k[0] = 1, t_i = float32(exp(-i*i / (2 sigma^2))) with libm's double exp, s = 1 + sum double(t_i * 2),
              k[i] = float32(k[i] * (1 / s));
  vertical    v = M[y][x] k[0]; for i = 1..m: v += (M[min(y+i,H-1)][x] + M[max(y-i,0)][x]) k[i]        (float32, each op rounded)
  horizontal  h = v[x] k[0];    for i = 1..m: h += k[i] (v[max(x-i,0)] + v[min(x+i,W-1)])
  solve       idet = 1 / (float64(g11 g22 - g12 g12) + 1e-3), flow = float32(float64(g11 h2 - g12 h1) idet), (g22 h1 - g12 h2) ..

Upstream interleaves a lagged stripe update of M with the row loop; it touches only rows that no later row's window
reads, so blurring the whole field and then updating the whole of M is the same computation (gauss_blur_solve_rows below
keeps upstream's interleaving; tests/test_gaussian_window_cpu.py compares the two).
"""
import math

import numpy as np

GAUSSIAN = 256   # cv2.OPTFLOW_FARNEBACK_GAUSSIAN


def _oracle():
    """The CPU oracle (what the `oracle` fixture of conftest.py returns)."""
    from oracle import oracle as O  # noqa: N812
    O.build()
    return O


def taps(winsize):
    m = winsize // 2
    sigma = m * 0.3
    k = np.zeros(m + 1, np.float32)
    k[0] = 1
    s = 1.0
    for i in range(1, m + 1):
        k[i] = np.float32(math.exp(-i * i / (2 * sigma * sigma)))
        s += float(k[i] * np.float32(2))
    s = 1. / s
    return np.array([np.float32(float(v) * s) for v in k], np.float32)


def _solve(h5):
    g11, g12, g22, h1, h2 = (h5[..., c] for c in range(5))
    idet = 1. / ((g11 * g22 - g12 * g12).astype(np.float64) + 1e-3)
    return np.stack([((g11 * h2 - g12 * h1).astype(np.float64) * idet).astype(np.float32),
                     ((g22 * h1 - g12 * h2).astype(np.float64) * idet).astype(np.float32)], axis=-1)


def _vertical(M, k, rows):
    """The vertical pass of rows `rows` of M [H][W][5] -> [len(rows)][W][5]."""
    H = M.shape[0]
    v = M[rows] * k[0]
    for i in range(1, len(k)):
        v = v + (M[np.minimum(rows + i, H - 1)] + M[np.maximum(rows - i, 0)]) * k[i]
    return v


def _horizontal(v, k):
    W = v.shape[1]
    xs = np.arange(W)
    h = v * k[0]
    for i in range(1, len(k)):
        h = h + k[i] * (v[:, np.maximum(xs - i, 0)] + v[:, np.minimum(xs + i, W - 1)])
    return h


def gauss_blur_solve(M_hw5, winsize):
    """M [H][W][5] float32 -> flow [H][W][2] float32 (both passes over the whole field, then the solve)."""
    M = np.ascontiguousarray(M_hw5, np.float32)
    assert M.ndim == 3 and M.shape[2] == 5 and winsize >= 2
    k = taps(winsize)
    with np.errstate(all="ignore"):
        return _solve(_horizontal(_vertical(M, k, np.arange(M.shape[0])), k))


def gauss_blur_solve_rows(R0, R1, flow, M, winsize, update):
    """Upstream's loop, row by row with its lagged stripe update of M -> (flow, M); the inputs are not modified."""
    oracle = _oracle()
    flow, M = np.array(flow, np.float32), np.array(M, np.float32)
    H, W = flow.shape[:2]
    k = taps(winsize)
    min_update_stripe = max((1 << 10) // W, winsize)
    y0 = 0
    for y in range(H):
        flow[y] = _solve(_horizontal(_vertical(M, k, np.array([y])), k))[0]
        y1 = H if y == H - 1 else y - winsize
        if update and (y1 == H or y1 >= y0 + min_update_stripe):
            oracle.update_matrices(R0, R1, flow, M, y0, y1)
            y0 = y1
    return flow, M


def farneback(prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, step):
    """FarnebackOpticalFlowImpl::calc composed from the oracle's stages; step(R0, R1, flow, M) -> the iteration's flow."""
    oracle = _oracle()
    h, w = prev.shape
    flow = None
    for k in range(oracle.effective_levels(w, h, pyr_scale, levels), -1, -1):
        wk, hk = oracle.level_geometry(w, h, pyr_scale, k)[:2]
        if flow is None:
            flow = np.zeros((hk, wk, 2), np.float32)
        else:
            flow = oracle.resize_linear(flow, wk, hk) * np.float32(1. / pyr_scale)
        R0 = oracle.polyexp(oracle.pyr_level(prev, pyr_scale, k), poly_n, poly_sigma)
        R1 = oracle.polyexp(oracle.pyr_level(nxt, pyr_scale, k), poly_n, poly_sigma)
        for _ in range(iterations):
            flow = step(R0, R1, flow, oracle.update_matrices(R0, R1, flow))
    return flow


def farneback_box(prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags=0):
    """The same composition with the oracle's box stage: must equal oracle.farneback (the scaffolding is the oracle's)."""
    assert flags == 0
    oracle = _oracle()
    return farneback(prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma,
                     lambda R0, R1, flow, M: oracle.update_flow_blur(R0, R1, flow, M, winsize, False)[0])


def farneback_gauss(prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags=GAUSSIAN):
    """The reference of a call with flags = 256."""
    assert flags == GAUSSIAN
    return farneback(prev, nxt, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma,
                     lambda R0, R1, flow, M: gauss_blur_solve(M, winsize))
