"""CPU: the accumulator oracle's correctly rounded mode (oracle/accum_ref.c, rounding="correct") pinned to mpmath at 50
digits, and still a faithful restatement of the reference (its goldens, at the tolerances of test_oracle_accum.py).

The device (accum_kernels.hip, pow_f32 / resistance_one) claims the correctly rounded float32 power and exp except within
~4e-14 of a rounding midpoint; tests/test_accum_cr_gpu.py holds it to this mode, so this mode must itself be exact."""
import math

import numpy as np
import pytest

from conftest import golden_path

mpmath = pytest.importorskip("mpmath")

F = np.float32
SOFF, SON, BOFF, BON = F(0.8), F(0.2), F(3.10), F(-5.12)
KOFF, KON, VOFF, VON, DT = F(51.03), F(-2.91), F(-0.2), F(0.1), F(5e-4)
RON, ROFF = 163305.0, 2104377.0
ONE_BITS = 0x3F800000
CASES = ["v1", "v2_split", "v2_magnitude", "v1_leak", "v2_split_bias", "v1_exact", "v2_split_pm1"]


def _mp():
    ctx = mpmath.mp.clone()
    ctx.dps = 50
    return ctx


MP = _mp()


def cr_f32(v):
    """mpf v (> 0) correctly rounded to float32: the nearest of the float32 neighbours of float(v)."""
    f = F(float(v))
    cands = (np.nextafter(f, F(0)), f, np.nextafter(f, F(np.inf)))
    return min(cands, key=lambda c: abs(MP.mpf(float(c)) - v))


def exact_pow(w, branch):
    """(1 - w*s)^b with the base formed in float32 as the oracle and the device do, the power exact, rounded once."""
    s, b = (SOFF, BOFF) if branch == 0 else (SON, BON)
    x = F(1) - np.asarray(w, F) * s
    ux, inv = np.unique(x, return_inverse=True)
    bb = MP.mpf(float(b))
    vals = np.array([cr_f32(MP.power(MP.mpf(float(v)), bb)) for v in ux], F)
    return vals[inv.reshape(x.shape)]


def update_from_pow(w, V, p):
    """update_one (event_mem_sim.py:40-57) in float32 around a given power term."""
    w, V = np.asarray(w, F), F(V)
    if V < VOFF:
        ka = KOFF * (V / VOFF - F(1))
    elif V > VON:
        ka = KON * (V / VON - F(1))
    else:
        return w.copy()
    return np.clip(w + (ka * p) * DT, F(0), F(1))


def bits(v):
    return int(np.array(v, F).view(np.uint32))


def around(centres, half=4096):
    """float32 w within +-half ulps of each centre, inside [0, 1]."""
    out = []
    for c in centres:
        b = bits(F(c))
        out.append(np.arange(max(0, b - half), min(ONE_BITS, b + half) + 1, dtype=np.uint32))
    return np.unique(np.concatenate(out)).view(F)


def edge_states():
    """0, 0.5, 1, every binade edge 2^-k, and the w where the device's series change regime: the base 1 - w*soff crossing
    sqrt(1/2) (and 2^-1.5, 0.5, 0.25: the split of frexp's mantissa, the exponent), and b * log(base) crossing
    (k + 1/2) ln 2, where exp_small's k changes."""
    c = [0.0, 0.5, 1.0] + [2.0 ** -k for k in range(1, 127)]
    for x in (2 ** -0.5, 2 ** -1.5, 0.5, 0.25):
        c.append((1 - x) / 0.8)
    for j in range(7):                       # soff branch: y = 3.1 ln x in [-4.99, 0]
        c.append((1 - 2 ** (-(j + 0.5) / 3.10)) / 0.8)
    for j in range(2):                       # son branch: y = -5.12 ln x in [0, 1.14]
        c.append((1 - 2 ** (-(j + 0.5) / 5.12)) / 0.2)
    return around([v for v in c if 0 <= v <= 1])


@pytest.mark.parametrize("branch", [0, 1])
def test_pow_random_states_vs_mpmath(oracle, branch):
    w = np.random.default_rng(20 + branch).random(100_000, dtype=F)
    got, flags = oracle.accum_pow(w, branch)
    assert np.array_equal(got, exact_pow(w, branch))
    assert not (flags & oracle.CR_UNDECIDED).any()


@pytest.mark.parametrize("branch", [0, 1])
def test_pow_edges_vs_mpmath(oracle, branch):
    w = edge_states()
    got, flags = oracle.accum_pow(w, branch)
    want = exact_pow(w, branch)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (w[bad[:5]], got[bad[:5]], want[bad[:5]])
    # and update_state around it, one V per branch: the oracle's float32 arithmetic around the power is update_one's
    V = F(-8.0) if branch == 0 else F(3.0)
    out, band = oracle.accum_update_state(w, np.full(w.shape, V), rounding="correct")
    assert np.array_equal(out, update_from_pow(w, V, want))
    assert np.array_equal(band, (flags & oracle.CR_BAND) != 0)


@pytest.mark.parametrize("branch", [0, 1])
def test_pow_long_double_cases_vs_mpmath(oracle, branch):
    """Every input of a strided sweep over [0, 1] on which the double pow lay within 2^-40 of a midpoint, so that powl
    decided: those are the inputs where a wrong fall-back would show."""
    w = np.arange(0, ONE_BITS + 1, 61, dtype=np.uint32).view(F)
    got, flags = oracle.accum_pow(w, branch)
    sel = (flags & oracle.CR_LONG) != 0
    assert sel.any()
    assert np.array_equal(got[sel], exact_pow(w[sel], branch))
    # the band is a subset of the long double cases, and rare
    assert not ((flags & oracle.CR_BAND) & ~flags & oracle.CR_LONG).any()
    assert (flags & oracle.CR_BAND).astype(bool).sum() < 1e-5 * w.size


def test_correct_mode_differs_from_libm_where_powf_misrounds(oracle):
    """The two modes are not the same function: glibc powf is off on ~5e-5 of the states, and on those the correct mode
    is the mpmath value."""
    w = np.arange(0, ONE_BITS + 1, 257, dtype=np.uint32).view(F)
    V = np.full(w.shape, -8.0, F)
    lm = oracle.accum_update_state(w, V)
    cr, _ = oracle.accum_update_state(w, V, rounding="correct")
    d = np.flatnonzero(lm != cr)
    assert 0 < d.size < 1e-3 * w.size
    assert np.array_equal(cr[d], update_from_pow(w[d], F(-8.0), exact_pow(w[d], 0)))


def _exact_resistance(w):
    neg_lam = F(-math.log(ROFF / RON))
    arg = neg_lam * (F(1) - np.asarray(w, F))
    e = np.array([cr_f32(MP.exp(MP.mpf(float(a)))) for a in arg.ravel()], F).reshape(arg.shape)
    return (RON / e.astype(np.float64)).astype(F)


def test_resistance_vs_mpmath(oracle):
    rng = np.random.default_rng(5)
    w = np.concatenate([rng.random(20_000, dtype=F), around([0.0, 0.5, 1.0], 512)])
    r, band = oracle.accum_resistance(w, rounding="correct")
    assert np.array_equal(r, _exact_resistance(w))
    assert band.sum() <= 2


def _gray_exact(b):
    """The "current" surface level of the float32 state with bit pattern b, from the exact chain."""
    w = np.array([b], np.uint32).view(F)
    r = _exact_resistance(w)[0]
    g = -3366 / MP.log10(1 / MP.mpf(float(r))) - 306
    return int(MP.floor(min(max(g, 0), 255)))


def _gray_state(b):
    w = np.array([b], np.uint32).view(F)
    return int(min(max(w[0] * F(255.0), 0), 255))


def _thresholds(gray):
    """{level: smallest float32 w in [0, 1] with gray(w) >= level} by bisection over bit patterns (gray is monotone)."""
    out = {}
    g0, g1 = gray(0), gray(ONE_BITS)
    for k in range(g0 + 1, g1 + 1):
        lo, hi = 0, ONE_BITS                 # gray(lo) < k <= gray(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if gray(mid) >= k:
                hi = mid
            else:
                lo = mid
        out[k] = hi
    return out


@pytest.mark.parametrize("mode", ["state", "current"])
def test_surface_thresholds_vs_mpmath(oracle, mode):
    """The 8-bit surface is a monotone step function of w: each of its level thresholds (255 in "state" mode, the 29
    above the level of w = 0 in "current" mode) computed exactly, and the oracle's map steps at exactly those floats."""
    gray = _gray_state if mode == "state" else _gray_exact
    th = _thresholds(gray)
    assert len(th) == (255 if mode == "state" else 255 - gray(0))
    levels = np.array(sorted(th), np.int64)
    at = np.array([th[k] for k in levels], np.uint32)
    g_at, band_at = oracle.accum_surface_u8(at.view(F), mode)
    g_below, band_below = oracle.accum_surface_u8((at - 1).view(F), mode)
    assert not band_at.any() and not band_below.any()
    assert np.array_equal(g_at, levels) and np.array_equal(g_below, levels - 1)
    # between the thresholds the map is flat: a dense sweep against the step function
    w = np.arange(0, ONE_BITS + 1, 4099, dtype=np.uint32)
    want = np.searchsorted(at, w, side="right") + (gray(0) if mode == "current" else 0)
    got, _ = oracle.accum_surface_u8(w.view(F), mode)
    assert np.array_equal(got, want)
    if mode == "current":
        f32, _ = oracle.accum_surface_f32(w.view(F), mode)
        assert np.array_equal(f32.astype(np.uint8), got)


def test_surface_f32_state_is_the_product(oracle):
    w = np.arange(0, ONE_BITS + 1, 997, dtype=np.uint32).view(F)
    f, band = oracle.accum_surface_f32(w, "state")
    assert np.array_equal(f, w * F(255.0)) and not band.any()


def test_correct_mode_against_reference_goldens(oracle):
    """The correct mode is still the reference's update: same goldens, same tolerances as the default mode."""
    g = np.load(golden_path("accum_update_state.npz"))
    for k in ("grid", "rand"):
        out, _ = oracle.accum_update_state(g[f"w_{k}"], g[f"V_{k}"], rounding="correct")
        assert np.abs(out - g[f"out_{k}"]).max() <= 1.2e-7
    r, _ = oracle.accum_resistance(g["w_rand"], rounding="correct")
    assert (np.abs(r - g["res_rand"]) / g["res_rand"]).max() <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_correct_mode_simulate_vs_reference(oracle, name):
    d = np.load(golden_path(f"accum_sim_{name}.npz"))
    H, W = d["w_final"].shape
    args = (d["x"], d["y"], d["p"], d["t"], H, W, int(d["version"]), str(d["polarity"]), int(d["slice_us"]),
            float(d["active_v"]), float(d["silent_v"]))
    out = oracle.accum_simulate(*args, rounding="correct")
    assert out["band"] >= 0
    assert np.abs(out["w_final"] - d["w_final"]).max() <= 3e-7
    idx = d["snap_idx"]
    assert (np.abs(out["resistances"][idx] - d["resistances"]) / d["resistances"]).max() <= 1e-6
    if "w_final_b" in d:
        assert np.abs(out["w_final_b"] - d["w_final_b"]).max() <= 3e-7
    # the default mode is untouched by the switch
    lm = oracle.accum_simulate(*args)
    assert "band" not in lm and np.abs(lm["w_final"] - out["w_final"]).max() <= 3e-7


def test_rounding_keyword_is_checked(oracle):
    with pytest.raises(ValueError):
        oracle.accum_update_state(np.zeros(1, F), np.zeros(1, F), rounding="nearest")
