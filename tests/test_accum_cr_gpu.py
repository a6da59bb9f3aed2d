"""GPU: the accumulator's float32 step functions against the oracle's correctly rounded mode, exhaustively over every
float32 state in [0, 1] (bit patterns 0 ... 0x3F800000), plus a sweep over the voltage and a table of inputs outside the
model.

accum_kernels.hip evaluates (1 - w*s)^b and exp(..) in double from series accurate to ~4e-14 and rounds once, so its
float32 results must equal the correctly rounded ones (oracle/accum_ref.c, rounding="correct") everywhere outside the
DEVICE BAND -- the inputs whose exact value lies within 2^-43 of a float32 rounding midpoint.  Inside the band either
neighbour is accepted; its size and the mismatches in it are reported (run with -s to see them)."""
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
KOFF, KON, VOFF, VON, DT = F(51.03), F(-2.91), F(-0.2), F(0.1), F(5e-4)
ONE_BITS = 0x3F800000
CHUNK = 1 << 26                      # states per chunk (256 MB of float32 on the host)
SUB = 1 << 24                        # states per accumulator run (4096 x 4096)
SIDE = 4096
V_OFF = (-8.0, -6.0, -1.0, -0.21)    # V < voff: (1 - 0.8 w)^3.1
V_ON = (0.11, 0.4, 1.0, 3.0)         # V > von: (1 - 0.2 w)^-5.12


def _pool():
    return ThreadPoolExecutor(min(16, len(os.sched_getaffinity(0))))


def _ptr(a, lo=0):
    return a.ctypes.data + lo * a.itemsize


def _par(pool, n, call):
    """call(lo, hi, counts) over pieces of [0, n) in the pool; the oracle's C loops release the GIL (ctypes).
    Returns the summed (band, undecided) counts."""
    step = max(1 << 16, -(-n // (4 * pool._max_workers)))
    pieces = [(lo, min(n, lo + step)) for lo in range(0, n, step)]
    counts = np.zeros((len(pieces), 2), np.int64)
    list(pool.map(lambda i: call(pieces[i][0], pieces[i][1], _ptr(counts[i])), range(len(pieces))))
    tot = counts.sum(0)
    assert tot[1] == 0, "oracle: correct rounding undecided in long double"
    return int(tot[0])


def _ka(V):
    V = F(V)
    return KOFF * (V / VOFF - F(1)) if V < VOFF else KON * (V / VON - F(1))


class Tally:
    """Per function: inputs checked, inputs in the device band, mismatches inside it, mismatches outside it."""

    def __init__(self):
        self.t = {}

    def add(self, name, n, band, bad_in, bad_out):
        r = self.t.setdefault(name, [0, 0, 0, 0])
        for i, v in enumerate((n, band, bad_in, bad_out)):
            r[i] += int(v)

    def report(self):
        for k, (n, band, bi, bo) in self.t.items():
            print(f"  {k:28s} inputs {n:11d}  band {band:6d}  mismatches in band {bi:4d}  outside {bo}")


def _cmp(tally, name, got, want, band):
    """got / want: torch tensors or numpy arrays of one dtype (compared bit for bit); band: bool of the same shape."""
    if not isinstance(got, np.ndarray):
        import torch
        it = torch.int32 if got.dtype == torch.float32 else got.dtype
        mism = got.view(it) != want.view(it)
        bad_in, bad_out = int((mism & band).sum()), int((mism & ~band).sum())
        nband = int(band.sum())
    else:
        it = np.int32 if got.dtype == F else got.dtype
        mism = got.view(it) != want.view(it)
        bad_in, bad_out = int((mism & band).sum()), int((mism & ~band).sum())
        nband = int(band.sum())
    tally.add(name, got.numel() if hasattr(got, "numel") else got.size, nband, bad_in, bad_out)
    return bad_out


def test_exhaustive_states_vs_correctly_rounded_oracle(nsof_lib, ctx, oracle, torch_dev):
    """Every float32 w in [0, 1] through
      update_one      (nsof_accum_update_state_dev) at V in {-8, -6, -1, -0.21, 0.11, 0.4, 1, 3}
      update_drive    the fused update of a one-slice Accumulator run after load_state: V as the silent voltage outside
                      the dead zone (the dense kernel's silent drive), and V as the active voltage with an event on every
                      pixel (the active drive)
      resistance_one  (nsof_accum_resistance_dev)
      the surface     surface_u8 and surface_f32, modes "current" and "state"
    equal to the correctly rounded oracle outside the device band."""
    import torch
    from nsof.accumulator import Accumulator
    from nsof.context import dev_ptr
    L = oracle.lib()
    lib = ctx._lib
    t_start = time.perf_counter()
    tally = Tally()
    bad = {}

    def fail(name, n):
        if n:
            bad[name] = bad.get(name, 0) + n

    # the accumulators of the fused checks, one geometry, reused across chunks
    xs = np.tile(np.arange(SIDE, dtype=np.int16), SIDE)
    ys = np.repeat(np.arange(SIDE, dtype=np.int16), SIDE)
    ev_all = (xs, ys, np.ones(SIDE * SIDE, np.int8), np.zeros(SIDE * SIDE, np.int64))
    ev_none = tuple(a[:0] for a in ev_all)
    silent, active = {}, {}
    for V in V_OFF + V_ON:
        a = Accumulator(SIDE, SIDE, 1, "split", -6.0, V, ctx=ctx)          # silent V outside the dead zone, no events
        a.set_events(*ev_none, np.array([0, 0], np.int64))
        silent[V] = a
        b = Accumulator(SIDE, SIDE, 1, "split", V, 0.0, ctx=ctx)           # active V, an event on every pixel
        b.set_events(*ev_all, np.array([0, SIDE * SIDE], np.int64))
        active[V] = b
    del xs, ys, ev_all
    surf = Accumulator(SIDE, SIDE, 1, "split", -6.0, 0.0, ctx=ctx)
    s_u8 = torch.empty((SIDE, SIDE), dtype=torch.uint8, device=torch_dev)
    s_f32 = torch.empty((SIDE, SIDE), dtype=torch.float32, device=torch_dev)

    def sub_states(w_h, lo, m):
        """w_h[lo:lo+m] as a SIDE x SIDE state (the tail padded with 0.5)."""
        st = np.full(SIDE * SIDE, 0.5, F)
        st[:m] = w_h[lo:lo + m]
        return st.reshape(SIDE, SIDE)

    try:
        with _pool() as pool:
            for c0 in range(0, ONE_BITS + 1, CHUNK):
                n = min(CHUNK, ONE_BITS + 1 - c0)
                w_h = np.arange(c0, c0 + n, dtype=np.uint32).view(F)
                w_d = torch.arange(c0, c0 + n, dtype=torch.int32, device=torch_dev).view(torch.float32)
                out = torch.empty_like(w_d)
                for branch, vs in ((0, V_OFF), (1, V_ON)):
                    p_h = np.empty(n, F)
                    fl_h = np.empty(n, np.uint8)
                    _par(pool, n, lambda lo, hi, c: L.nsof_ref_accum_pow_cr(_ptr(w_h, lo), branch, _ptr(p_h, lo),
                                                                             _ptr(fl_h, lo), hi - lo, c))
                    band_h = (fl_h & oracle.CR_BAND) != 0
                    del fl_h
                    p_d = torch.from_numpy(p_h).to(torch_dev)
                    del p_h
                    band_d = torch.from_numpy(band_h).to(torch_dev)
                    dt_d = torch.tensor(DT, dtype=torch.float32, device=torch_dev)
                    for V in vs:
                        # the oracle's update_one around its power, float32 products and sum in update_one's order
                        ka_d = torch.tensor(_ka(V), dtype=torch.float32, device=torch_dev)
                        ref = torch.clamp(w_d + (ka_d * p_d) * dt_d, 0.0, 1.0)
                        v_d = torch.full_like(w_d, V)
                        torch.cuda.synchronize()
                        ctx.check(lib.nsof_accum_update_state_dev(ctx.ptr, dev_ptr(w_d), dev_ptr(v_d), dev_ptr(out), n),
                                  "update_state_dev")
                        ctx.synchronize()
                        fail(f"update_one V={V}", _cmp(tally, f"update_one V={V}", out, ref, band_d))
                        del v_d
                        ref_h = ref.cpu().numpy()
                        del ref
                        for acc, what in ((silent[V], "silent"), (active[V], "active")):
                            name = f"update_drive {what} V={V}"
                            for lo in range(0, n, SUB):
                                m = min(SUB, n - lo)
                                acc.load_state(dict(w=sub_states(w_h, lo, m)))
                                acc.run(0, 1)
                                got = acc.w().ravel()[:m]
                                fail(name, _cmp(tally, name, got, ref_h[lo:lo + m], band_h[lo:lo + m]))
                        del ref_h
                    del p_d, band_d, band_h
                # resistance
                r_h = np.empty(n, F)
                fl_h = np.empty(n, np.uint8)
                _par(pool, n, lambda lo, hi, c: L.nsof_ref_accum_resistance_cr(_ptr(w_h, lo), _ptr(r_h, lo),
                                                                                _ptr(fl_h, lo), hi - lo, c))
                torch.cuda.synchronize()
                ctx.check(lib.nsof_accum_resistance_dev(ctx.ptr, dev_ptr(w_d), dev_ptr(out), n), "resistance_dev")
                ctx.synchronize()
                fail("resistance_one", _cmp(tally, "resistance_one", out, torch.from_numpy(r_h).to(torch_dev),
                                            torch.from_numpy((fl_h & oracle.CR_BAND) != 0).to(torch_dev)))
                del r_h, fl_h, out, w_d
                # the surface, both outputs, both modes
                for mode, m_i in (("current", 0), ("state", 1)):
                    g8 = np.empty(n, np.uint8)
                    g32 = np.empty(n, F)
                    f8 = np.empty(n, np.uint8)
                    f32 = np.empty(n, np.uint8)
                    _par(pool, n, lambda lo, hi, c: L.nsof_ref_accum_surface(_ptr(w_h, lo), hi - lo, m_i, _ptr(g8, lo),
                                                                              None, _ptr(f8, lo), c))
                    _par(pool, n, lambda lo, hi, c: L.nsof_ref_accum_surface(_ptr(w_h, lo), hi - lo, m_i, None,
                                                                              _ptr(g32, lo), _ptr(f32, lo), c))
                    for lo in range(0, n, SUB):
                        m = min(SUB, n - lo)
                        surf.load_state(dict(w=sub_states(w_h, lo, m)))
                        torch.cuda.synchronize()
                        surf.surface_u8(s_u8, mode=mode)
                        surf.surface_f32(s_f32, mode=mode)
                        ctx.synchronize()
                        got8 = s_u8.cpu().numpy().ravel()[:m]
                        got32 = s_f32.cpu().numpy().ravel()[:m]
                        fail(f"surface_u8 {mode}", _cmp(tally, f"surface_u8 {mode}", got8, g8[lo:lo + m],
                                                        (f8[lo:lo + m] & oracle.CR_BAND) != 0))
                        fail(f"surface_f32 {mode}", _cmp(tally, f"surface_f32 {mode}", got32, g32[lo:lo + m],
                                                         (f32[lo:lo + m] & oracle.CR_BAND) != 0))
                    del g8, g32, f8, f32
                del w_h
    finally:
        for a in list(silent.values()) + list(active.values()) + [surf]:
            a.close()
    print(f"\nexhaustive sweep over {ONE_BITS + 1} states: {time.perf_counter() - t_start:.1f} s")
    tally.report()
    assert all(r[0] >= ONE_BITS + 1 for r in tally.t.values())
    assert not bad, f"mismatches outside the device band: {bad}"


def test_voltage_sweep_vs_correctly_rounded_oracle(nsof_lib, ctx, oracle):
    """Every 97th float32 V in [-10, 10] (both signs), voff, von, their neighbours and +-0, at w in {0, 2^-24, 0.5,
    1 - 2^-24, 1}: update_one equals the correctly rounded oracle outside the device band."""
    top = int(np.array(10.0, F).view(np.uint32))
    pos = np.arange(0, top + 1, 97, dtype=np.uint32)
    V = np.concatenate([pos, pos | np.uint32(0x80000000)]).view(F)
    extra = [F(-0.2), F(0.1), F(0.0), F(-0.0)]
    extra += [np.nextafter(v, F(s)) for v in (F(-0.2), F(0.1)) for s in (-1, 1)]
    V = np.concatenate([V, np.array(extra, F)])
    L = oracle.lib()
    tally = Tally()
    with _pool() as pool:
        for w0 in (F(0), F(2.0 ** -24), F(0.5), F(1) - F(2.0 ** -24), F(1)):
            w = np.full(V.shape, w0, F)
            want = np.empty_like(w)
            fl = np.empty(w.shape, np.uint8)
            _par(pool, w.size, lambda lo, hi, c: L.nsof_ref_accum_update_state_cr(_ptr(w, lo), _ptr(V, lo), _ptr(want, lo),
                                                                                   _ptr(fl, lo), hi - lo, c))
            got = nsof_lib.update_state(w, V, ctx=ctx)
            _cmp(tally, f"update_one w={float(w0)!r}", got, want, (fl & oracle.CR_BAND) != 0)
            # the dead zone [voff, von] (thresholds exclusive) leaves w unchanged, bit for bit
            dz = (V >= F(-0.2)) & (V <= F(0.1))
            assert np.array_equal(got[dz], w[dz])
    tally.report()
    assert all(r[3] == 0 for r in tally.t.values()), tally.t


def _numpy_update(w, V):
    """event_mem_sim.py:40-57 in NumPy float32 (its own float32 power)."""
    dwdt = np.zeros_like(w)
    off, on = V < VOFF, V > VON
    with np.errstate(all="ignore"):
        dwdt[off] = KOFF * (V[off] / VOFF - F(1)) * (F(1) - w[off] * F(0.8)) ** F(3.10)
        dwdt[on] = KON * (V[on] / VON - F(1)) * (F(1) - w[on] * F(0.2)) ** F(-5.12)
        return np.clip(w + dwdt * DT, F(0), F(1))


def test_out_of_model_states_follow_numpy_semantics(nsof_lib, ctx, oracle):
    """The element-wise entry on states outside [0, 1]: negative w, 1.25 (base 0 of the soff branch), 5 (negative base),
    NaN, +-inf, denormals.  The device gives what NumPy's float32 update gives: NaN exactly where NumPy has NaN, the
    special values (0, 1, inf bases) exactly, the finite rest the correctly rounded value."""
    w = np.array([-1.0, -0.5, -1e-30, -0.0, 1.25, 5.0, np.nan, np.inf, -np.inf, 1e-45, 1e-40, -1e-40, 1e-38, 2.5, -3e38,
                  3e38], F)
    for v in (-8.0, -0.21, 0.05, 0.11, 3.0):
        V = np.full(w.shape, v, F)
        got = nsof_lib.update_state(w, V, ctx=ctx)
        want, band = oracle.accum_update_state(w, V, rounding="correct")
        ref = _numpy_update(w, V)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (v, w, got, ref)
        ok = ~np.isnan(ref) & ~band
        assert np.array_equal(got[ok].view(np.int32), want[ok].view(np.int32)), (v, w[ok], got[ok], want[ok])
        # and within an ulp of NumPy's own float32 power (not correctly rounded) where finite
        from conftest import ulp_diff
        assert ulp_diff(got[ok], ref[ok]).max() <= 2, (v, got[ok], ref[ok])
