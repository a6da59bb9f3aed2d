// The float32 event-driven accumulator: what accum_kernels.hip (one array) and accum_trials.hip (T Monte-Carlo trials of one
// stream) share.  Device code: the update arithmetic (update_one, Drive, drive_of, update_drive, replay_driven,
// resistance_one, surface_gray_value), the scatter of a group of slices (k_scatter and its marks), scheme 1's count threshold (Theta,
// driven_bits), scheme 2's refractory walk (RefrTab, refractory_walk), the set-up pass of per-pixel devices (k_setup_maps)
// the resistance read-outs (k_resistance, k_block_min_resistance) and the check and slice times of a stream that lies in
// device memory (k_stream_check, k_slice_times).  Host code: the staged stream (StagedStream: stage, stage_dev) and the
// walk over its groups (group_len, snapshot_due, refr_tab_of, ListCounts).  Everything sits in an unnamed namespace, as in
// accum_model.h: each translation unit instantiates its own copies.
#pragma once

#include <type_traits>
#include <vector>

#include "accum_model.h"

namespace {

constexpr int MAX_GROUP = 32;

// x ** b for the float32 state update, evaluated in double and rounded once (NumPy's float32 power is accurate to
// about an ulp; this is correctly rounded except within ~1e-13 of a rounding boundary).  The library log()/exp() spend
// most of their ~150 double-precision instructions on ranges and special cases that cannot occur here
// (x = 1 - w*s lies in [0.2, 1] for a state in [0, 1]); the series below need ~55 and are accurate to 4e-14:
//   log: x = m * 2^e with m in [sqrt(1/2), sqrt(2)), z = (m-1)/(m+1), log m = 2z(1 + z^2/3 + ... + z^14/15)
//   exp: y = k ln2 + r with |r| <= ln2/2, exp r = sum r^n/n! (n <= 13), scaled by 2^k
__device__ __forceinline__ double log_unit_range(double x)
{
    int e;
    double m = frexp(x, &e);                       // m in [0.5, 1)
    if (m < 0.70710678118654752440) { m *= 2.0; e -= 1; }
    const double z = (m - 1.0) / (m + 1.0), w = z * z;
    double p = 1.0 / 15.0;
    p = fma(p, w, 1.0 / 13.0);
    p = fma(p, w, 1.0 / 11.0);
    p = fma(p, w, 1.0 / 9.0);
    p = fma(p, w, 1.0 / 7.0);
    p = fma(p, w, 1.0 / 5.0);
    p = fma(p, w, 1.0 / 3.0);
    p = fma(p, w, 1.0);
    const double de = (double)e;
    return fma(de, 0x1.62e42feep-1, fma(de, 0x1.a39ef35793c76p-33, 2.0 * z * p));   // e * ln2 in two parts
}
__device__ __forceinline__ double exp_small(double y)   // |y| < 700
{
    const double k = rint(y * 1.4426950408889634074);
    const double r = fma(-k, 0x1.a39ef35793c76p-33, fma(-k, 0x1.62e42feep-1, y));
    double p = 1.0 / 6227020800.0;
    p = fma(p, r, 1.0 / 479001600.0);
    p = fma(p, r, 1.0 / 39916800.0);
    p = fma(p, r, 1.0 / 3628800.0);
    p = fma(p, r, 1.0 / 362880.0);
    p = fma(p, r, 1.0 / 40320.0);
    p = fma(p, r, 1.0 / 5040.0);
    p = fma(p, r, 1.0 / 720.0);
    p = fma(p, r, 1.0 / 120.0);
    p = fma(p, r, 1.0 / 24.0);
    p = fma(p, r, 1.0 / 6.0);
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    return ldexp(p, (int)k);
}
__device__ __forceinline__ float pow_f32(float x, float b)
{
    // A state outside [0,1] handed to the element-wise entry point can make x <= 0 or non-finite; the result then follows
    // np.power on float32 operands (C99 powf): x ** 0 = 1 for every x, NaN included; a finite negative base gives nan for a
    // non-integer exponent and (-1)^b |x|^b for an integer one; the bases 0 and -inf give 0 or inf by the sign of b, and
    // carry the base's sign for an odd integer b.  (A float of magnitude >= 2^24 is an even integer.)
    if (!(x > 0.f)) {
        if (b == 0.f) return 1.f;
        if (x != x) return x;
        const bool whole = truncf(b) == b, odd = whole && fabsf(b) < 16777216.f && ((long long)b & 1);
        if (x == 0.f || x == -__builtin_inff()) {
            const float r = ((x == 0.f) == (b > 0.f)) ? 0.f : __builtin_inff();
            return odd ? copysignf(r, x) : r;
        }
        if (!whole) return __builtin_nanf("");
        const float r = (float)exp((double)b * log((double)-x));
        return odd ? -r : r;
    }
    // The library path: a base far outside the model's range (1 - w*s lies in [0.2, 1] for the fitted device; another
    // device's s may reach 0), or an exponent beyond 100 -- exp_small wants |b ln x| < 700, and |ln x| <= 6.91 on [1e-3, 2].
    // The test on b is uniform: a scalar compare.
    if (x > 2.f || x < 1e-3f || !(fabsf(b) <= 100.f)) return b == 0.f ? 1.f : (float)exp((double)b * log((double)x));
    return (float)exp_small((double)b * log_unit_range((double)x));
}

// k * (V/v0 - 1) ** alpha: the first product of the reference's "k * A**alpha * B**b".  alpha == 1 (the fitted device) calls
// no pow: x ** 1 is x.
__device__ __forceinline__ float drive_gain(float V, float v0, float k, float alpha)
{
    const float a = V / v0 - 1.f;
    return k * (alpha == 1.f ? a : pow_f32(a, alpha));
}

__device__ __forceinline__ float update_one(float w, float V, const DevF& p)
{
    float dwdt = 0.f;
    if (V < p.voff) {
        const float b = pow_f32(1.f - w * p.soff, p.boff);
        dwdt = drive_gain(V, p.voff, p.koff, p.alphaoff) * b;
    } else if (V > p.von) {
        const float b = pow_f32(1.f - w * p.son, p.bon);
        dwdt = drive_gain(V, p.von, p.kon, p.alphaon) * b;
    }
    const float wn = w + dwdt * p.dt;
    return wn < 0.f ? 0.f : (wn > 1.f ? 1.f : wn);
}

// A slice's voltage is one of two values per run (active / silent), so everything of update_one that depends on V
// alone is evaluated once: the branch taken, k * (V/v0 - 1) ** alpha (the first product of "k * A**alpha * B**b", same
// rounding; the power, where alpha != 1, once per voltage and never per slice), and the (s, b) pair of the power term.  The
// per-slice step is then branch-free: one pow, two multiplies, one add, the clip.
struct Drive {
    // dead zone: ka = 0 and the power term is (1 - w*0) ** 1 = 1 whatever the device's s and b, so dw = 0 * 1 = 0 and a finite
    // w is unchanged bit for bit, as in update_one (a term like (1 - w*s) ** b could overflow for another device: 0 * inf)
    float ka, s, b, dt;
};
__device__ __forceinline__ Drive drive_of(float V, const DevF& p)
{
    Drive d;
    d.dt = p.dt;
    if (V < p.voff) { d.ka = drive_gain(V, p.voff, p.koff, p.alphaoff); d.s = p.soff; d.b = p.boff; }
    else if (V > p.von) { d.ka = drive_gain(V, p.von, p.kon, p.alphaon); d.s = p.son; d.b = p.bon; }
    else { d.ka = 0.f; d.s = 0.f; d.b = 1.f; }
    return d;
}
__device__ __forceinline__ float update_drive(float w, const Drive& d)
{
    const float wn = w + (d.ka * pow_f32(1.f - w * d.s, d.b)) * d.dt;
    return wn < 0.f ? 0.f : (wn > 1.f ? 1.f : wn);
}

// resistance_exp: Ron / exp(-lam * (1 - w)), every operand float32 as NumPy makes them (the quotient of two floats formed in
// double and rounded once is the float32 quotient)
__device__ __forceinline__ float resistance_one(float w, const DevF& p)
{
    const float e = (float)exp((double)(p.neg_lam * (1.0f - w)));
    return (float)((double)p.ron / (double)e);
}

// The surface value of one pixel before its 8-bit truncation: g in [0, 255], double (modes: see k_surface_gray).
__device__ __forceinline__ double surface_gray_value(float ww, const DevF& p, int mode)
{
    double g;
    if (mode == 0) {
        const double r = (double)resistance_one(ww, p);
        g = -3366.0 / log10(1.0 / r) - 306.0;
    } else {
        g = (double)(ww * 255.0f);
    }
    g = g < 0.0 ? 0.0 : (g > 255.0 ? 255.0 : g);   // NaN (I == 1 A exactly, R == 1 Ohm) does not occur for the fitted R in [Ron, Roff]
    return g;
}
// The surface as an 8-bit frame, one pixel.
__device__ __forceinline__ uint8_t surface_gray_one(float ww, const DevF& p, int mode)
{
    return (uint8_t)surface_gray_value(ww, p, mode);
}

// A pixel's drive and resistance constants from the planes k_setup_maps wrote.
__device__ __forceinline__ Drive drive_at(const float* __restrict__ plane, size_t pix, float dt)
{
    const float* q = plane + 3 * pix;
    return Drive{q[0], q[1], q[2], dt};
}

// Largest s in [0, n_sl) with bounds[s] <= e: the slice of event e.  bounds = event indices of the slice boundaries
// (n_sl + 1 entries).
__device__ __forceinline__ int slice_of(const long long* bounds, int n_sl, long long e)
{
    int lo = 0, hi = n_sl;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (bounds[mid] <= e) lo = mid; else hi = mid;
    }
    return lo;
}

// Marks (pixel, slice bit) in a mask of 32- or 64-bit words; a pixel's first touch in this group enters the compact list
// once, so no two threads of the list update ever hold the same pixel.  The list's counter is ONE word: appended to per lane
// it serialises every first touch of a group at the L2 atomic unit (~10 ns each: 300 us for the 33 k events of a 32-slice
// group at 1 M events/s, found with rocprofv3), so the appends of a wave are aggregated -- one atomicAdd of the wave's
// count, ranks from the ballot.  Call with the whole wave (inactive lanes pass active = false); list == nullptr
// (every-pixel update: no list is read) skips the list entirely.
__device__ __forceinline__ void list_append(unsigned* list, unsigned* count, unsigned pix, bool first)
{
    const unsigned long long b = __ballot(first);
    if (!b) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)b) - 1;
    unsigned base = 0;
    if (lane == leader) base = atomicAdd(count, (unsigned)__popcll(b));
    base = __shfl(base, leader);
    if (first) list[base + (unsigned)__popcll(b & ((1ull << lane) - 1ull))] = pix;
}
template <class MaskT>
__device__ __forceinline__ void mark(MaskT* mask, unsigned* list, unsigned* count, unsigned pix, MaskT bit, bool active)
{
    const MaskT old = active ? atomicOr(&mask[pix], bit) : (MaskT)1;
    if (!list) return;
    list_append(list, count, pix, active && old == 0);
}

// Scheme 1's event-count threshold (THETA_EVENTS of event_mem_sim.py:33, :208-217: a pixel pulses in a slice when
// bincount_2d(x[sl], y[sl]) >= theta).  theta == 1 is the mask bit above.  theta > 1: the same mask word holds one saturating
// counter of `bits` = ceil(log2(theta + 1)) bits per slice instead of one bit, so a 32-bit word carries spw = 32 / bits
// slices of a group and a 64-bit word 64 / bits; a compare-and-swap loop adds 1 and stops at theta, so a field never
// carries into its neighbour however many events the cell receives (theta <= INT32_MAX: bits <= 31).  "old word == 0" is
// still the pixel's first touch in the group -- a count of 1 makes the word non-zero -- so the list append is mark's; the
// update kernels turn fields into driven bits (field == theta) as they load the word and clear it as they always did: no
// plane, no launch and no clearing step is added, and a group simply holds fewer slices.
struct Theta {
    int theta, bits, spw;   // spw: slices per 32-bit word
};
struct NoTheta {};
template <bool COUNT>
using ThetaArg = std::conditional_t<COUNT, Theta, NoTheta>;   // theta == 1 passes nothing: the instantiations it always ran

// One event of (pixel, the slice whose field starts at bit `shift`).
template <class MaskT>
__device__ __forceinline__ void mark_count(MaskT* mask, unsigned* list, unsigned* count, unsigned pix, int shift, const Theta& th,
                                           bool active)
{
    MaskT old = 1;
    if (active) {
        const MaskT fm = ((MaskT)1 << th.bits) - 1, one = (MaskT)1 << shift;
        // a stale value costs a retry and nothing else: fields only grow within a group, so "saturated" stays true, and
        // the first touch is decided by the compare-and-swap that replaces 0
        MaskT cur = __hip_atomic_load(&mask[pix], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        for (;;) {
            old = cur;
            if (((cur >> shift) & fm) >= (MaskT)th.theta) break;   // saturated (cur != 0: no first touch)
            const MaskT seen = atomicCAS(&mask[pix], cur, cur + one);
            if (seen == cur) break;
            cur = seen;
        }
    }
    if (!list) return;
    list_append(list, count, pix, active && old == 0);
}

// Counter fields of a mask word -> one bit per slice whose count reached theta (bit s = the word's s-th field).
template <class MaskT>
__device__ __forceinline__ MaskT driven_bits(MaskT f, const Theta& th)
{
    const MaskT fm = ((MaskT)1 << th.bits) - 1;
    MaskT m = 0;
    for (int s = 0; f; s++, f >>= th.bits)
        if ((f & fm) >= (MaskT)th.theta) m |= (MaskT)1 << s;
    return m;
}

// One scatter per group of slices, both schemes: every event marks (pixel, its slice) in its array's mask.
//   split == 0  every event -> array 0 (scheme 1 :208-217, scheme 2 magnitude; p is not read)
//   split == 1  p == 1 -> array 0, p == 0 -> array 1 (:238, :250; other polarity values drive nothing)
// Slices 32..63 of a group (scheme 1's every-pixel update only: n_sl <= 32 otherwise) go to the second mask word mask_hi.
//   COUNT  scheme 1 with theta > 1 (no split): the event counts into its slice's field (mark_count); slices th.spw..2 * th.spw - 1
//          of a group are the second word's
template <bool COUNT>
__global__ __launch_bounds__(256) void k_scatter(const short* __restrict__ x, const short* __restrict__ y,
                                                  const signed char* __restrict__ p, long long ev0, long long n_ev,
                                                  const long long* __restrict__ bounds, int n_sl, int W, int split,
                                                  unsigned* mask0, unsigned* list0, unsigned* count0, unsigned* mask1,
                                                  unsigned* list1, unsigned* count1, unsigned* mask_hi, ThetaArg<COUNT> th)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n_ev;
    const long long e = ev0 + (live ? i : 0);
    int arr = 0;
    if (split) {
        const int pv = (int)p[e];
        arr = pv == 1 ? 0 : (pv == 0 ? 1 : -1);
    }
    const int s = slice_of(bounds, n_sl, e);
    if constexpr (COUNT) {
        const unsigned pix = (unsigned)y[e] * (unsigned)W + (unsigned)x[e];
        const bool hi = s >= th.spw;
        mark_count(hi ? mask_hi : mask0, list0, count0, pix, (hi ? s - th.spw : s) * th.bits, th, live);
    } else {
        const unsigned pix = (unsigned)y[e] * (unsigned)W + (unsigned)x[e], bit = 1u << (s & 31);
        mark(s < 32 ? mask0 : mask_hi, list0, count0, pix, bit, live && arr == 0);
        if (split) mark(mask1, list1, count1, pix, bit, live && arr == 1);
    }
}

// Scheme 2's refractory rule (event_mem_sim.py:237-269) looks like a chain over slices -- slice s+1 tests the next_ok that
// slice s wrote -- but the chain is PER PIXEL: a pixel's next_ok depends on that pixel's own earlier events only, and within a
// slice every event of a pixel sees the same next_ok (NumPy reads next_ok[ys, xs] before it writes).  So a group of up to 32
// slices needs ONE scatter, "which slices have an event (of the array's polarity) at this pixel" (bit s of E), and the
// eligibility walk moves into the fused state update: per touched pixel, over the set bits of E in slice order,
//     if next_ok <= t_first[s]:  the pixel is driven in slice s;  next_ok = t_last[s] + REFRACTORY
// with the per-slice constants in a 64-entry table.  No atomics on next_ok, two launches per group and array as in scheme 1.
struct RefrTab {
    long long t_first[32], t_next[32];
};
struct NoTab {};
template <bool REFR>
using TabArg = std::conditional_t<REFR, RefrTab, NoTab>;   // scheme 1 passes no table

// slices with an event -> slices in which the pixel is driven; ok = the pixel's next_ok (updated)
__device__ __forceinline__ unsigned refractory_walk(unsigned e, long long& ok, const long long* tf, const long long* tn)
{
    unsigned m = 0;
    for (; e; e &= e - 1) {
        const int s = __ffs((int)e) - 1;
        if (ok <= tf[s]) {
            m |= 1u << s;
            ok = tn[s];
        }
    }
    return m;
}

// The active drive once per set bit of m: the driven slices of a pixel in slice order (the silent ones are no-ops).
template <class MaskT>
__device__ __forceinline__ float replay_driven(float ww, MaskT m, const Drive& da)
{
    for (; m; m &= m - 1) ww = update_drive(ww, da);
    return ww;
}

inline int grid_for(size_t n, int cap = 4096)
{
    size_t g = (n + 255) / 256;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? cap : g));
}

// The counter layout of a threshold: bits = ceil(log2(theta + 1)) per slice (theta >= 1, at most 31 bits).
inline Theta theta_of(int theta)
{
    int bits = 1;
    while ((1ll << bits) < (long long)theta + 1) bits++;
    return Theta{theta, bits, 32 / bits};
}
// f(std::false_type, NoTheta) for theta == 1, f(std::true_type, Theta) for a count threshold
template <class Fn>
void with_theta(int theta, Fn&& f)
{
    if (theta == 1) f(std::false_type{}, NoTheta{});
    else f(std::true_type{}, theta_of(theta));
}

// ---- per-pixel (and per-trial) devices: the set-up pass ---------------------------------------------------------------
// The planes as the set-up pass reads them: the value of key k at (trial t, pixel i) is plane[k][t * stride[k] + i]
// (stride 0: one plane shared by the trials) or, without a plane, scalar[k].
struct MapSrc {
    const float* plane[NSOF_ACCUM_KEY_COUNT];   // nullptr: the key is uniform
    size_t stride[NSOF_ACCUM_KEY_COUNT];
    float scalar[NSOF_ACCUM_KEY_COUNT];
    double ron, roff;                           // the scalars' doubles
    float dt;
};
// Once per nsof_accum_set_param_maps / nsof_accum_trials_dev call, per (trial = blockIdx.y, pixel): the DevF of that pixel --
// a mapped key's float32 value, an unmapped one's scalar -- and from it exactly what the uniform kernels form per launch:
// drive_of at the two voltages and (ron, neg_lam), neg_lam = (float)(-ln(Roff / Ron)) with the logarithm in double of the
// values as held (a plane's float32 widened, the scalar's double).
//   drive_trials  the trials that get drives and a resistance pair: all, or 1 when no plane but wini has a trial axis
//   sil           nullptr where no kernel reads the silent drive (the trial run's touched-pixels form)
//   w0, w1        the initial state (the trial's wini) of every array; nullptr where nsof_accum_reset sets it (one array)
//   v_act_t, v_sil_t  the two voltages per trial ([drive_trials] each, both or neither); nullptr: v_act / v_sil for all
__global__ __launch_bounds__(256) void k_setup_maps(MapSrc src, size_t n, int drive_trials, float v_act, float v_sil,
                                                     float* __restrict__ act, float* __restrict__ sil, float2* __restrict__ res,
                                                     float* __restrict__ w0, float* __restrict__ w1,
                                                     const float* __restrict__ v_act_t, const float* __restrict__ v_sil_t)
{
    const size_t t = blockIdx.y;
    if (v_act_t && t < (size_t)drive_trials) {
        v_act = v_act_t[t];
        v_sil = v_sil_t[t];
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        auto get = [&](int k) { return src.plane[k] ? src.plane[k][t * src.stride[k] + i] : src.scalar[k]; };
        const size_t e = t * n + i;
        if (w0) {
            const float wini = get(NSOF_ACCUM_KEY_WINI);
            w0[e] = wini;
            if (w1) w1[e] = wini;
        }
        if (t >= (size_t)drive_trials) continue;
        DevF p;
        p.alphaoff = get(NSOF_ACCUM_KEY_ALPHAOFF); p.alphaon = get(NSOF_ACCUM_KEY_ALPHAON);
        p.voff = get(NSOF_ACCUM_KEY_VOFF); p.von = get(NSOF_ACCUM_KEY_VON);
        p.koff = get(NSOF_ACCUM_KEY_KOFF); p.kon = get(NSOF_ACCUM_KEY_KON);
        p.son = get(NSOF_ACCUM_KEY_SON); p.soff = get(NSOF_ACCUM_KEY_SOFF);
        p.bon = get(NSOF_ACCUM_KEY_BON); p.boff = get(NSOF_ACCUM_KEY_BOFF);
        p.dt = src.dt;
        p.ron = get(NSOF_ACCUM_KEY_RON);
        const double ron = src.plane[NSOF_ACCUM_KEY_RON] ? (double)p.ron : src.ron;
        const double roff = src.plane[NSOF_ACCUM_KEY_ROFF] ? (double)get(NSOF_ACCUM_KEY_ROFF) : src.roff;
        p.neg_lam = (float)(-log(roff / ron));
        const Drive da = drive_of(v_act, p);
        act[3 * e] = da.ka; act[3 * e + 1] = da.s; act[3 * e + 2] = da.b;
        if (sil) {
            const Drive ds = drive_of(v_sil, p);
            sil[3 * e] = ds.ka; sil[3 * e + 1] = ds.s; sil[3 * e + 2] = ds.b;
        }
        res[e] = make_float2(p.ron, p.neg_lam);
    }
}
// The checked planes to device memory (dplane[k], on ctx->stream; the caller's arrays must outlive the copies) and the MapSrc
// of them: the model's float32 scalars for the unmapped keys.
inline int upload_planes(nsof_ctx* ctx, const Model& mo, const PlaneSet<float>& ps, size_t npx, nsof_dev_buf<float>* dplane, MapSrc* src)
{
    const float scal[NSOF_ACCUM_KEY_COUNT] = {mo.f.alphaoff, mo.f.alphaon, mo.f.voff, mo.f.von, mo.f.koff, mo.f.kon, mo.f.son, mo.f.soff,
                                              mo.f.bon, mo.f.boff, mo.f.ron, (float)mo.prm.Roff, mo.wini_f};
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++) {
        src->plane[k] = nullptr;
        src->stride[k] = 0;
        src->scalar[k] = scal[k];
        if (!ps.plane[k]) continue;
        const size_t bytes = (size_t)ps.trials[k] * npx * sizeof(float);
        if (int rc = dplane[k].reserve(ctx, bytes)) return rc;
        NSOF_HIP(ctx, hipMemcpyAsync(dplane[k].p, ps.plane[k], bytes, hipMemcpyHostToDevice, ctx->stream));
        src->plane[k] = dplane[k].p;
        src->stride[k] = ps.trials[k] > 1 ? npx : 0;
    }
    src->ron = mo.prm.Ron;
    src->roff = mo.prm.Roff;
    src->dt = mo.f.dt;
    return NSOF_OK;
}

// ---- resistance ---------------------------------------------------------------------------------------------------------
// The model resistance_one / surface_gray_value read (ron, neg_lam; mode 1 of the surface reads neither: no load): the
// uniform device itself, pixel pix of a mapped one, or element i of the trial run's [A][T][npx] states.
struct MapRes {
    const float2* res;
};
struct TrialRes {
    const float2* res;   // [T or 1][npx]
    size_t stride, npx;  // stride: float2s between the planes of consecutive trials (0: one plane for all)
    int n_trials;
};
__device__ __forceinline__ const DevF& res_at(const DevF& p, size_t, int) { return p; }
__device__ __forceinline__ DevF res_at(const float2* __restrict__ res, size_t pix, int mode)
{
    DevF q{};
    if (mode == 0) {
        const float2 r = res[pix];
        q.ron = r.x;
        q.neg_lam = r.y;
    }
    return q;
}
__device__ __forceinline__ DevF res_at(MapRes m, size_t pix, int mode) { return res_at(m.res, pix, mode); }
__device__ __forceinline__ DevF res_at(const TrialRes& v, size_t i, int mode)
{
    return res_at(v.res + (i / v.npx % (size_t)v.n_trials) * v.stride, i % v.npx, mode);
}

//   ResT  DevF (one device), MapRes (element i is pixel i of a mapped accumulator) or TrialRes
template <class ResT>
__global__ __launch_bounds__(256) void k_resistance(const float* __restrict__ w, float* __restrict__ out, size_t n, ResT p)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = resistance_one(w[i], res_at(p, i, 0));
}

// Block maximum of the device current I = v_ds / R over memsize x memsize pixel blocks: the gating image's input
// (one value per block) formed on the device instead of from a downloaded surface.
// max(v_ds / R) = v_ds / min(R) exactly (division by a positive float is monotone), so a block reduces min(R) in
// float32 -- R from a stored snapshot, or resistance_one(w) of the current state -- and thread 0 divides in double.
//   ResT        DevF, MapRes or TrialRes: the resistance constants, read where the source is the state
//   blockIdx.z  the trial: its plane of src starts at z * src_stride floats, its map of out at z * out_stride doubles (one
//               array: z = 0)
template <class ResT>
__global__ __launch_bounds__(256) void k_block_min_resistance(const float* __restrict__ src, int is_w, int W, int memsize,
                                                               int cols, ResT p, double v_ds, double* __restrict__ out,
                                                               size_t src_stride, size_t out_stride)
{
    __shared__ float part[4];
    const int bx = blockIdx.x, by = blockIdx.y;
    const size_t base = blockIdx.z * src_stride + ((size_t)by * memsize) * W + (size_t)bx * memsize;
    float m = INFINITY;
    for (int i = threadIdx.x; i < memsize * memsize; i += 256) {
        const size_t pix = base + (size_t)(i / memsize) * W + (i % memsize);
        const float v = src[pix];
        m = fminf(m, is_w ? resistance_one(v, res_at(p, pix, 0)) : v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        out[blockIdx.z * out_stride + (size_t)by * cols + bx] = v_ds / (double)fminf(fminf(part[0], part[1]), fminf(part[2], part[3]));
}

// ---- a stream in device memory: its check and its slice times ------------------------------------------------------------
// The record a check leaves, 64-bit words: [0] the verdict -- the smallest index of an event at fault, all ones for none --,
// [1] t[e0] and [2] t[e1 - 1] (ORDER only), [3] unused.  The host sets the verdict to all ones before the launch.
constexpr int STREAM_REC = 4;
constexpr unsigned long long STREAM_CLEAN = ~0ull;

// One pass over events [e0, e1) of a device stream.  At fault is an event
//   XY     whose coordinates lie outside the W x H sensor (x, y are read)
//   ORDER  e > e0 whose time lies before its predecessor's (t is read, and its two ends go to the record)
// A wave walks 64 consecutive events per step, so the first set bit of its ballot is the wave's smallest index of that step
// and, the steps ascending, of the whole walk: that lane issues the wave's ONE atomic minimum and the wave leaves.
template <bool XY, bool ORDER>
__global__ __launch_bounds__(256) void k_stream_check(const short* __restrict__ x, const short* __restrict__ y,
                                                       const long long* __restrict__ t, long long e0, long long e1, int W, int H,
                                                       unsigned long long* rec)
{
    const int lane = threadIdx.x & 63;
    const long long stride = (long long)gridDim.x * 256;
    for (long long e = e0 + (long long)blockIdx.x * 256 + threadIdx.x; e - lane < e1; e += stride) {   // (the test is the wave's)
        bool bad = false;
        if (e < e1) {
            if constexpr (XY) bad = (unsigned)x[e] >= (unsigned)W || (unsigned)y[e] >= (unsigned)H;
            if constexpr (ORDER) {
                const long long te = t[e];
                bad = bad || (e > e0 && te < t[e - 1]);
                if (e == e0) rec[1] = (unsigned long long)te;
                if (e == e1 - 1) rec[2] = (unsigned long long)te;
            }
        }
        const unsigned long long b = __ballot(bad);
        if (b) {
            if (lane == __ffsll((long long)b) - 1) atomicMin(&rec[0], (unsigned long long)e);
            break;
        }
    }
}
// Scheme 2's two times per slice s of a device stream, as StagedStream::stage forms them on the host: t of the slice's first
// event and t of its last + the refractory period, zeros for an empty slice.  rel: the n_slices + 1 bounds relative to e0.
__global__ __launch_bounds__(256) void k_slice_times(const long long* __restrict__ t, long long e0, const long long* __restrict__ rel,
                                                      long long n_slices, long long refractory_us, long long* __restrict__ tfirst,
                                                      long long* __restrict__ tnext)
{
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= n_slices) return;
    const long long a = rel[s], b = rel[s + 1];
    const bool live = b > a;
    tfirst[s] = live ? t[e0 + a] : 0;
    tnext[s] = live ? t[e0 + b - 1] + refractory_us : 0;
}

// The context's words for such a stream (device, and the pinned twin the copies go through): at least `words` of each.
inline int stream_words(nsof_ctx* ctx, size_t words)
{
    const size_t bytes = words * sizeof(long long), cap = align_up(bytes + bytes / 2, 4096);
    if (int rc = ctx->evtab.reserve(ctx, bytes, cap)) return rc;
    return ctx->evtab_h.reserve(ctx, bytes, cap);
}

// ---- the staged stream and the walk over its groups (host) --------------------------------------------------------------
// The events of slices [0, n_slices) on the device and what the slice loop needs of them on the host: the slice bounds
// relative to the first staged event and, for scheme 2, every slice's first timestamp and last timestamp + refractory period.
struct StagedStream {
    std::vector<long long> rel, tfirst, tnext;   // (declared first: the buffers below wait for the device as they go)
    nsof_dev_buf<short> dx, dy;
    nsof_dev_buf<signed char> dp;
    nsof_dev_buf<long long> dbounds;
    // What refuses a stream whatever memory its events lie in: the bounds and the arrays that must be there.
    static int check_bounds(nsof_ctx* ctx, int scheme, int split, bool have_xyt, bool have_p, const int64_t* sb, int64_t n_slices)
    {
        if (n_slices < 0 || !sb) return nsof_set_error(ctx, NSOF_EINVAL, "bad slice bounds");
        const int64_t n_ev = sb[n_slices] - sb[0];
        if (n_ev < 0) return nsof_set_error(ctx, NSOF_EINVAL, "slice bounds not monotone");
        if (n_ev > 0 && (!have_xyt || (scheme == 2 && split && !have_p))) return nsof_set_error(ctx, NSOF_EINVAL, "null event array");
        for (int64_t s = 0; s < n_slices; s++)
            if (sb[s + 1] < sb[s]) return nsof_set_error(ctx, NSOF_EINVAL, "slice bounds not monotone");
        return NSOF_OK;
    }
    // ... and the refusal of event e at (x, y), the first in stream order outside the sensor
    static int refuse_event(nsof_ctx* ctx, int64_t e, int x, int y, int W, int H)
    {
        return nsof_set_error(ctx, NSOF_EINVAL, "event %lld at (%d,%d) outside the %dx%d sensor", (long long)e, x, y, W, H);
    }
    // Everything about a stream that refuses it, on the host: nothing is allocated, uploaded or launched.
    static int check(nsof_ctx* ctx, int W, int H, int scheme, int split, const int16_t* x, const int16_t* y, const int8_t* p,
                     const int64_t* t, const int64_t* sb, int64_t n_slices)
    {
        if (int rc = check_bounds(ctx, scheme, split, x && y && t, p != nullptr, sb, n_slices)) return rc;
        // validate coordinates on the host: an out-of-range event would be an out-of-bounds store on the device
        for (int64_t e = sb[0]; e < sb[n_slices]; e++)
            if ((unsigned)x[e] >= (unsigned)W || (unsigned)y[e] >= (unsigned)H) return refuse_event(ctx, e, x[e], y[e], W, H);
        return NSOF_OK;
    }
    // stage() for a stream that lies in DEVICE memory: d_x, d_y, d_p, d_t hold n_events events, sb (host) indexes them.  The
    // check runs on the device (k_stream_check) and its verdict comes back, with scheme 2's slice times, in one copy:
    // the first wait.  Only then is anything of this object written -- a refused stream leaves the staged one as it was --
    // and the events are copied device to device.  Across PCIe go the bounds (8 B per slice, up), the record (32 B) and
    // scheme 2's times (16 B per slice, down).  The caller's arrays are read until ctx->stream has drained: the caller's
    // wait, the second.
    int stage_dev(nsof_ctx* ctx, int W, int H, int scheme, int split, long long refractory_us, const int16_t* d_x, const int16_t* d_y,
                  const int8_t* d_p, const int64_t* d_t, int64_t n_events, const int64_t* sb, int64_t n_slices)
    {
        if (int rc = check_bounds(ctx, scheme, split, d_x && d_y && d_t, d_p != nullptr, sb, n_slices)) return rc;
        const int64_t e0 = sb[0], e1 = sb[n_slices], n_ev = e1 - e0;
        if (e0 < 0 || e1 > n_events)
            return nsof_set_error(ctx, NSOF_EINVAL, "slice bounds [%lld, %lld] outside the %lld events of the device stream", (long long)e0,
                                  (long long)e1, (long long)n_events);
        NSOF_HIP(ctx, hipSetDevice(ctx->device));
        // the words: rel [ns + 1], the record [STREAM_REC], tfirst [ns], tnext [ns]
        const size_t ns = (size_t)n_slices, rec = ns + 1, tf = rec + STREAM_REC, tn = tf + ns;
        if (int rc = stream_words(ctx, tn + ns)) return rc;
        long long *const h = ctx->evtab_h.p, *const d = ctx->evtab.p;
        for (size_t s = 0; s <= ns; s++) h[s] = (long long)(sb[s] - e0);
        NSOF_HIP(ctx, hipMemcpyAsync(d, h, rec * 8, hipMemcpyHostToDevice, ctx->stream));
        const bool times = scheme == 2 && n_ev > 0;
        if (n_ev > 0) {
            NSOF_HIP(ctx, hipMemsetAsync(d + rec, 0xFF, 8, ctx->stream));
            hipLaunchKernelGGL((k_stream_check<true, false>), dim3(grid_for((size_t)n_ev)), dim3(256), 0, ctx->stream, (const short*)d_x,
                               (const short*)d_y, (const long long*)nullptr, (long long)e0, (long long)e1, W, H,
                               reinterpret_cast<unsigned long long*>(d + rec));
            if (times)
                hipLaunchKernelGGL(k_slice_times, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, ctx->stream, (const long long*)d_t,
                                   (long long)e0, (const long long*)d, (long long)n_slices, refractory_us, d + tf, d + tn);
            NSOF_HIP(ctx, hipGetLastError());
            NSOF_HIP(ctx, hipMemcpyAsync(h + rec, d + rec, (STREAM_REC + (times ? 2 * ns : 0)) * 8, hipMemcpyDeviceToHost, ctx->stream));
            NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
            if ((unsigned long long)h[rec] != STREAM_CLEAN) {   // (the refusal's own two reads are not part of the count above)
                const int64_t e = (int64_t)h[rec];
                int16_t bx = 0, by = 0;
                NSOF_HIP(ctx, hipMemcpyAsync(&bx, d_x + e, 2, hipMemcpyDeviceToHost, ctx->stream));
                NSOF_HIP(ctx, hipMemcpyAsync(&by, d_y + e, 2, hipMemcpyDeviceToHost, ctx->stream));
                NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
                return refuse_event(ctx, e, bx, by, W, H);
            }
        }
        int rc;
        const size_t cap = event_cap(n_ev);
        if ((rc = dx.reserve(ctx, (size_t)n_ev * 2, cap * 2)) || (rc = dy.reserve(ctx, (size_t)n_ev * 2, cap * 2)) ||
            (rc = dp.reserve(ctx, (size_t)n_ev, cap)) || (rc = dbounds.reserve(ctx, rec * 8)))
            return rc;
        if (n_ev > 0) {
            NSOF_HIP(ctx, hipMemcpyAsync(dx.p, d_x + e0, (size_t)n_ev * 2, hipMemcpyDeviceToDevice, ctx->stream));
            NSOF_HIP(ctx, hipMemcpyAsync(dy.p, d_y + e0, (size_t)n_ev * 2, hipMemcpyDeviceToDevice, ctx->stream));
            if (d_p) NSOF_HIP(ctx, hipMemcpyAsync(dp.p, d_p + e0, (size_t)n_ev, hipMemcpyDeviceToDevice, ctx->stream));
        }
        NSOF_HIP(ctx, hipMemcpyAsync(dbounds.p, d, rec * 8, hipMemcpyDeviceToDevice, ctx->stream));
        rel.assign(h, h + rec);
        if (times) {
            tfirst.assign(h + tf, h + tf + ns);
            tnext.assign(h + tn, h + tn + ns);
        } else {
            tfirst.assign(ns, 0);
            tnext.assign(ns, 0);
        }
        return NSOF_OK;
    }
    // Checks and uploads on ctx->stream (bounds sb index the caller's arrays, which are not retained: synchronise before
    // they go).  checked: the caller has run check() on these very arguments.
    int stage(nsof_ctx* ctx, int W, int H, int scheme, int split, long long refractory_us, const int16_t* x, const int16_t* y,
              const int8_t* p, const int64_t* t, const int64_t* sb, int64_t n_slices, bool checked = false)
    {
        if (!checked)
            if (int rc = check(ctx, W, H, scheme, split, x, y, p, t, sb, n_slices)) return rc;
        NSOF_HIP(ctx, hipSetDevice(ctx->device));
        const int64_t e0 = sb[0], e1 = sb[n_slices], n_ev = e1 - e0;
        int rc;
        const size_t cap = event_cap(n_ev);
        if ((rc = dx.reserve(ctx, (size_t)n_ev * 2, cap * 2)) || (rc = dy.reserve(ctx, (size_t)n_ev * 2, cap * 2)) ||
            (rc = dp.reserve(ctx, (size_t)n_ev, cap)) || (rc = dbounds.reserve(ctx, (size_t)(n_slices + 1) * 8)))
            return rc;
        if (n_ev > 0) {
            NSOF_HIP(ctx, hipMemcpyAsync(dx.p, x + e0, (size_t)n_ev * 2, hipMemcpyHostToDevice, ctx->stream));
            NSOF_HIP(ctx, hipMemcpyAsync(dy.p, y + e0, (size_t)n_ev * 2, hipMemcpyHostToDevice, ctx->stream));
            if (p) NSOF_HIP(ctx, hipMemcpyAsync(dp.p, p + e0, (size_t)n_ev, hipMemcpyHostToDevice, ctx->stream));
        }
        rel.resize((size_t)n_slices + 1);
        for (int64_t s = 0; s <= n_slices; s++) rel[s] = (long long)(sb[s] - e0);
        tfirst.assign((size_t)n_slices, 0);
        tnext.assign((size_t)n_slices, 0);
        if (scheme == 2)
            for (int64_t s = 0; s < n_slices; s++)
                if (sb[s + 1] > sb[s]) {
                    tfirst[s] = t[sb[s]];
                    tnext[s] = t[sb[s + 1] - 1] + refractory_us;
                }
        NSOF_HIP(ctx, hipMemcpyAsync(dbounds.p, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        return NSOF_OK;
    }
    // entries an event-sized buffer is given so that a slightly longer stream reuses it
    static size_t event_cap(int64_t n_ev) { return (size_t)n_ev + (size_t)n_ev / 4 + 1024; }
};

// The next group: up to max_group slices of [s0, s_end), ending right after the next snapshot slice (`counter`: the slices
// run since the array was reset, which times the snapshots).
inline int64_t group_len(int64_t s0, int64_t s_end, int64_t max_group, int64_t snap_every, int64_t counter)
{
    int64_t g = s_end - s0 < max_group ? s_end - s0 : max_group;
    if (snap_every > 0) {
        const int64_t to_snap = (counter % snap_every == 0) ? 1 : (snap_every - counter % snap_every) + 1;
        if (to_snap < g) g = to_snap;
    }
    return g;
}
// ... and whether the group that brought the counter here ended on one
inline bool snapshot_due(int64_t counter, int64_t snap_every) { return snap_every > 0 && (counter - 1) % snap_every == 0; }
// Scheme 2's table of the group of g <= 32 slices from s0 (an empty slice drives nothing: zeros)
inline RefrTab refr_tab_of(const StagedStream& st, int64_t s0, int64_t g)
{
    RefrTab tab;
    for (int s = 0; s < 32; s++) {
        const bool live = s < g && st.rel[s0 + s + 1] > st.rel[s0 + s];
        tab.t_first[s] = live ? st.tfirst[s0 + s] : 0;
        tab.t_next[s] = live ? st.tnext[s0 + s] : 0;
    }
    return tab;
}

// List counters of the event-pixel update, [parity][array]: two sets used alternately.  A group's update kernels zero the
// OTHER set -- the one the next group's scatter appends to -- so no group needs a memset (a launch of its own): one per call.
struct ListCounts {
    unsigned* base;
    int par = 0;
    hipError_t zero_all(hipStream_t s) const { return hipMemsetAsync(base, 0, 4 * sizeof(unsigned), s); }
    unsigned* cur() const { return base + 2 * par; }
    unsigned* next() const { return base + 2 * (par ^ 1); }
    void flip() { par ^= 1; }
};

}  // namespace
