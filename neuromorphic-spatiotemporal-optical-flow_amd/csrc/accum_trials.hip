// Event-driven accumulator, Monte-Carlo device trials: ONE staged stream drives T arrays whose devices differ (per-pixel,
// per-trial parameter planes) in one run -- nsof_accum_trials_dev.  The float32 arithmetic is accum_update.h's, the one
// the single-array path (accum_kernels.hip) runs: trial t gives, bit for bit, what an accumulator with trial t's planes
// (nsof_accum_set_param_maps) gives on the same stream.
//
// What cannot differ between trials is done once.  Which slices drive which pixel depends on the events alone -- scheme
// 1 compares a pixel's per-slice event count with theta, scheme 2 walks the event times against the pixel's next_ok, and
// neither reads a device parameter -- so per group of up to 32 slices (th.spw with a count threshold), cut at the snapshot
// slices exactly as the single-array path cuts them:
//   k_scatter          (accum_update.h, unchanged) the group's events -> per-pixel mask words + the list of touched pixels
//   k_trials_resolve   one thread per listed pixel: counter fields -> driven bits, scheme 2's refractory walk (ONE next_ok
//                      plane per array, not T), the mask word cleared, the driven word stored parallel to the list, the
//                      other parity's list counter zeroed.  Here the ownership of the mask word and of next_ok ends, so
//   k_trials_update    may spread over (list chunks x trial chunks) without a race: per (trial, listed pixel) it loads
//                      w[t][pix] and the pixel's active drive (12 B), replays the driven slices and stores w: 20 B per
//                      listed pixel and trial, plus the 8 B of (pixel, driven word) once per TRIAL_CHUNK trials.
// That form needs silent_v in the dead zone of EVERY pixel of EVERY trial (an idle pixel is then a bit-exact no-op).
// Otherwise k_trials_update_all visits every pixel with its per-trial silent drive: one thread per pixel owns the mask
// word and next_ok and walks the T trials itself -- the plain form; leaking arrays are not what the trial run is for.
// k_trials_setup is k_setup_maps with a trial axis (and the initial state), k_trials_block_current is
// k_block_min_resistance's reduction with one, taken from the state at the snapshot slices: no full-resolution snapshot
// stack exists.
#include <algorithm>
#include <cmath>
#include <vector>

#include "accum_update.h"

namespace {

constexpr int TRIAL_CHUNK = 4;       // trials per thread of k_trials_update
constexpr int MAX_TRIALS = 65535;    // the trial axis is a grid dimension

// The planes as the set-up pass reads them: the value of key k at (trial t, pixel i) is plane[k][t * stride[k] + i]
// (stride 0: one plane shared by the trials) or, without a plane, scalar[k].
struct TrialSrc {
    const float* plane[NSOF_ACCUM_KEY_COUNT];
    size_t stride[NSOF_ACCUM_KEY_COUNT];
    float scalar[NSOF_ACCUM_KEY_COUNT];
    double ron, roff;   // the scalars' doubles
    float dt;
};

// Per (trial, pixel): the initial state (the trial's wini) of every array and, for the first drive_trials trials, what
// k_setup_maps forms per pixel -- drive_of at the two voltages and (ron, neg_lam), neg_lam = (float)(-ln(Roff / Ron)) with the
// logarithm in double of the values as held.  drive_trials is T, or 1 when no plane but wini has a trial axis.
//   sil  nullptr where no kernel reads the silent drive (the touched-pixels form)
__global__ __launch_bounds__(256) void k_trials_setup(TrialSrc src, size_t n, int drive_trials, float v_act, float v_sil,
                                                       float* __restrict__ act, float* __restrict__ sil, float2* __restrict__ res,
                                                       float* __restrict__ w0, float* __restrict__ w1)
{
    const size_t t = blockIdx.y;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        auto get = [&](int k) { return src.plane[k] ? src.plane[k][t * src.stride[k] + i] : src.scalar[k]; };
        const size_t e = t * n + i;
        const float wini = get(NSOF_ACCUM_KEY_WINI);
        w0[e] = wini;
        if (w1) w1[e] = wini;
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

// The group's refractory table in LDS (scheme 2), as the single-array update kernels hold it.
template <bool REFR>
struct RefrLds {
    long long tf[REFR ? 32 : 1], tn[REFR ? 32 : 1];
};
template <bool REFR>
__device__ __forceinline__ void load_tab(RefrLds<REFR>& l, const TabArg<REFR>& tab)
{
    if constexpr (REFR) {
        if (threadIdx.x < 32) { l.tf[threadIdx.x] = tab.t_first[threadIdx.x]; l.tn[threadIdx.x] = tab.t_next[threadIdx.x]; }
        __syncthreads();
    }
}
// A pixel's mask word -> the slices of the group in which it is driven (every trial alike); claims next_ok.
template <bool REFR, bool COUNT>
__device__ __forceinline__ unsigned resolve_one(unsigned m, long long* __restrict__ next_ok, size_t pix, const RefrLds<REFR>& l,
                                                const ThetaArg<COUNT>& th)
{
    if constexpr (COUNT) m = driven_bits(m, th);
    if constexpr (REFR) {
        if (m) {
            long long ok = next_ok[pix];
            m = refractory_walk(m, ok, l.tf, l.tn);
            if (m) next_ok[pix] = ok;
        }
    }
    return m;
}

template <bool REFR, bool COUNT>
__global__ __launch_bounds__(256) void k_trials_resolve(unsigned* __restrict__ mask, long long* __restrict__ next_ok,
                                                         const unsigned* __restrict__ list, const unsigned* __restrict__ count,
                                                         TabArg<REFR> tab, unsigned* __restrict__ driven, unsigned* zero_next,
                                                         ThetaArg<COUNT> th)
{
    __shared__ RefrLds<REFR> l;
    load_tab<REFR>(l, tab);
    const unsigned n = *count;
    if (blockIdx.x == 0 && threadIdx.x == 0) *zero_next = 0;   // the NEXT group's list counter (other parity)
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned pix = list[i];
        const unsigned m = mask[pix];
        mask[pix] = 0;
        driven[i] = resolve_one<REFR, COUNT>(m, next_ok, pix, l, th);
    }
}

// blockIdx.y: a chunk of TRIAL_CHUNK trials.  act_stride: floats between the drive planes of consecutive trials (0: one
// plane for all).  Nothing here is shared between trial chunks but the read-only list and driven words.
__global__ __launch_bounds__(256) void k_trials_update(float* __restrict__ w, const unsigned* __restrict__ list,
                                                        const unsigned* __restrict__ count, const unsigned* __restrict__ driven,
                                                        const float* __restrict__ act, size_t act_stride, size_t npx, int n_trials,
                                                        float dt)
{
    const unsigned n = *count;
    const int t0 = blockIdx.y * TRIAL_CHUNK;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned m = driven[i];
        if (!m) continue;   // no slice of the group drives the pixel: every trial's state stays
        const size_t pix = list[i];
        float ww[TRIAL_CHUNK];
        Drive d[TRIAL_CHUNK];
#pragma unroll
        for (int k = 0; k < TRIAL_CHUNK; k++)
            if (t0 + k < n_trials) {
                ww[k] = w[(size_t)(t0 + k) * npx + pix];
                d[k] = drive_at(act + (size_t)(t0 + k) * act_stride, pix, dt);
            }
#pragma unroll
        for (int k = 0; k < TRIAL_CHUNK; k++)
            if (t0 + k < n_trials) w[(size_t)(t0 + k) * npx + pix] = replay_driven(ww[k], m, d[k]);
    }
}

// The every-pixel form: silent_v outside the dead zone of some pixel of some trial.  One thread per pixel resolves the
// pixel's mask word once and replays all n_sl slices of the group for each trial with that trial's two drives (a pixel whose
// own dead zone holds silent_v carries the no-op drive, ka = 0), as k_update_all does for one mapped array.
template <bool REFR, bool COUNT>
__global__ __launch_bounds__(256) void k_trials_update_all(float* __restrict__ w, unsigned* __restrict__ mask,
                                                            long long* __restrict__ next_ok, size_t npx, int n_sl, TabArg<REFR> tab,
                                                            const float* __restrict__ act, const float* __restrict__ sil,
                                                            size_t drive_stride, int n_trials, float dt, ThetaArg<COUNT> th)
{
    __shared__ RefrLds<REFR> l;
    load_tab<REFR>(l, tab);
    for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < npx; pix += (size_t)gridDim.x * 256) {
        unsigned m = mask[pix];
        if (m) mask[pix] = 0;
        m = resolve_one<REFR, COUNT>(m, next_ok, pix, l, th);
        for (int t = 0; t < n_trials; t++) {
            const Drive pa = drive_at(act + (size_t)t * drive_stride, pix, dt), ps = drive_at(sil + (size_t)t * drive_stride, pix, dt);
            float ww = w[(size_t)t * npx + pix];
            for (int s = 0; s < n_sl; s++) ww = update_drive(ww, (m >> s) & 1u ? pa : ps);
            w[(size_t)t * npx + pix] = ww;
        }
    }
}

__device__ __forceinline__ float trial_resistance(float w, float2 r)
{
    DevF q{};
    q.ron = r.x;
    q.neg_lam = r.y;
    return resistance_one(w, q);
}

// resistance_one of every (array, trial, pixel): w is [A][T][npx], res [T or 1][npx].
__global__ __launch_bounds__(256) void k_trials_resistance(const float* __restrict__ w, const float2* __restrict__ res,
                                                            size_t res_stride, size_t npx, int n_trials, size_t total,
                                                            float* __restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pix = i % npx, t = i / npx % (size_t)n_trials;
        out[i] = trial_resistance(w[i], res[t * res_stride + pix]);
    }
}

// Block maximum of the device current v_ds / R of one array's T states (blockIdx.z: the trial): min(R) over the memsize x
// memsize block in float32, one division in double -- what nsof_accum_block_current_dev forms from a stored snapshot of
// resistance_one(w).  out points at this array's [T][n_snaps][rows][cols]; the launch fills snapshot `snap` of every trial.
__global__ __launch_bounds__(256) void k_trials_block_current(const float* __restrict__ w, const float2* __restrict__ res,
                                                               size_t res_stride, size_t npx, int W, int memsize, int cols,
                                                               size_t snap, size_t n_snaps, double v_ds, double* __restrict__ out)
{
    __shared__ float part[4];
    const int bx = blockIdx.x, by = blockIdx.y;
    const size_t t = blockIdx.z;
    const size_t base = ((size_t)by * memsize) * W + (size_t)bx * memsize;
    float m = INFINITY;
    for (int i = threadIdx.x; i < memsize * memsize; i += 256) {
        const size_t pix = base + (size_t)(i / memsize) * W + (i % memsize);
        m = fminf(m, trial_resistance(w[t * npx + pix], res[t * res_stride + pix]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0)
        out[((t * n_snaps + snap) * gridDim.y + by) * cols + bx] = v_ds / (double)fminf(fminf(part[0], part[1]), fminf(part[2], part[3]));
}

// The caller's planes by key: plane[k] (nullptr: the key is uniform) holds trials[k] trials, 1 or n_trials.
struct TrialPlanes {
    const float* plane[NSOF_ACCUM_KEY_COUNT] = {};
    int trials[NSOF_ACCUM_KEY_COUNT] = {};
};

}  // namespace

extern "C" int nsof_accum_trials_dev(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v,
                                     float silent_v, const nsof_accum_params* params, int theta, const int16_t* x, const int16_t* y,
                                     const int8_t* p, const int64_t* t, const int64_t* sb, int64_t n_slices, int64_t snap_every,
                                     int memsize, double v_ds, int n_trials, int n_maps, const int* keys, const float* const* planes,
                                     const int* plane_trials, float* d_w, float* d_resistance, double* d_block_current)
{
    if (!ctx) return NSOF_EINVAL;
    // ---- everything that can refuse the call, on the host, before anything is allocated, uploaded or launched
    if (!d_w || !d_resistance) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: NULL output");
    if (height < 1 || width < 1 || (scheme != 1 && scheme != 2))
        return nsof_set_error(ctx, NSOF_EINVAL, "bad accumulator geometry %dx%d or scheme %d", height, width, scheme);
    if (theta < 1) return nsof_set_error(ctx, NSOF_EINVAL, "event threshold %d: at least 1 event", theta);
    if (scheme == 2 && theta != 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "event threshold %d: scheme 2 has no count threshold (only 1 is accepted)", theta);
    if (n_trials < 1) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: %d trials (at least 1)", n_trials);
    if (n_maps < 0 || n_maps > NSOF_ACCUM_KEY_COUNT || (n_maps > 0 && (!keys || !planes || !plane_trials)))
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: %d maps (0..%d, with their keys, planes and trial counts)", n_maps,
                              NSOF_ACCUM_KEY_COUNT);
    TrialPlanes tp;
    for (int j = 0; j < n_maps; j++) {
        const int k = keys[j];
        if (k < 0 || k >= NSOF_ACCUM_KEY_COUNT)
            return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: key %d is no parameter (0..%d)", k, NSOF_ACCUM_KEY_COUNT - 1);
        if (!planes[j]) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: the plane of %s is NULL", kKeyNames[k]);
        if (tp.plane[k]) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: %s given twice", kKeyNames[k]);
        if (plane_trials[j] != 1 && plane_trials[j] != n_trials)
            return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: the plane of %s holds %d trials (1 or %d)", kKeyNames[k],
                                  plane_trials[j], n_trials);
        tp.plane[k] = planes[j];
        tp.trials[k] = plane_trials[j];
    }
    Model mo;
    if (int rc = model_of(ctx, params, &mo)) return rc;
    const bool blocks = d_block_current != nullptr;
    if (blocks && (snap_every < 1 || memsize < 1 || memsize > width || memsize > height || !(v_ds > 0)))
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: block currents need snap_every >= 1 (%lld), 1 <= memsize <= %d (%d), v_ds > 0 (%g)",
                              (long long)snap_every, std::min(width, height), memsize, v_ds);
    if (n_slices < 1 || !sb) return nsof_set_error(ctx, NSOF_EINVAL, "bad slice bounds");
    const int64_t e0 = sb[0], n_ev = sb[n_slices] - e0;
    if (n_ev < 0) return nsof_set_error(ctx, NSOF_EINVAL, "slice bounds not monotone");
    const int split = (scheme == 2 && polarity_split) ? 1 : 0, narr = split ? 2 : 1;
    if (n_ev > 0 && (!x || !y || !t || (split && !p))) return nsof_set_error(ctx, NSOF_EINVAL, "null event array");
    for (int64_t s = 0; s < n_slices; s++)
        if (sb[s + 1] < sb[s]) return nsof_set_error(ctx, NSOF_EINVAL, "slice bounds not monotone");
    // an out-of-range event would be an out-of-bounds store on the device
    for (int64_t e = e0; e < e0 + n_ev; e++)
        if ((unsigned)x[e] >= (unsigned)width || (unsigned)y[e] >= (unsigned)height)
            return nsof_set_error(ctx, NSOF_EINVAL, "event %lld at (%d,%d) outside the %dx%d sensor", (long long)e, (int)x[e], (int)y[e],
                                  width, height);
    const size_t npx = (size_t)height * width, T = (size_t)n_trials;
    // the domain of model_of, per pixel of every plane of every trial, in the order the planes were given
    for (int j = 0; j < n_maps; j++)
        for (size_t e = 0; e < (size_t)plane_trials[j] * npx; e++)
            if (const char* why = key_value_refused(keys[j], planes[j][e]))
                return nsof_set_error(ctx, NSOF_EINVAL, "trial parameter map %s: trial %zu, row %zu, column %zu = %g %s", kKeyNames[keys[j]],
                                      e / npx, e % npx / (size_t)width, e % (size_t)width, (double)planes[j][e], why);
    const int lam_trials = std::max(tp.trials[NSOF_ACCUM_KEY_RON], tp.trials[NSOF_ACCUM_KEY_ROFF]);
    for (size_t tr = 0; tr < (size_t)lam_trials; tr++) {
        const float* const pon = tp.plane[NSOF_ACCUM_KEY_RON] ? tp.plane[NSOF_ACCUM_KEY_RON] + (tp.trials[NSOF_ACCUM_KEY_RON] == 1 ? 0 : tr) * npx : nullptr;
        const float* const poff = tp.plane[NSOF_ACCUM_KEY_ROFF] ? tp.plane[NSOF_ACCUM_KEY_ROFF] + (tp.trials[NSOF_ACCUM_KEY_ROFF] == 1 ? 0 : tr) * npx : nullptr;
        for (size_t i = 0; i < npx; i++) {
            // (ln q is finite exactly for a finite q > 0 -- subnormal q included: decided without T * H * W logarithms)
            const double q = (poff ? (double)poff[i] : mo.prm.Roff) / (pon ? (double)pon[i] : mo.prm.Ron);
            if (!(q > 0 && std::isfinite(q)))
                return nsof_set_error(ctx, NSOF_EINVAL, "trial parameter maps Ron / Roff: ln(Roff / Ron) is not finite at trial %zu, row %zu, column %zu",
                                      tr, i / (size_t)width, i % (size_t)width);
        }
    }
    if (npx > 0xFFFFFFFFull) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "sensor too large");
    if (n_trials > MAX_TRIALS || n_ev >= (1ll << 31))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%d trials of %zu pixels, %lld events: too large for one launch", n_trials, npx,
                              (long long)n_ev);
    // silent_v inside the dead zone of EVERY pixel of EVERY trial (the float32 comparisons update_one makes): the
    // touched-pixels form; otherwise the every-pixel form
    // (the two thresholds are tested independently, so each plane is one flat pass)
    auto every_value = [&](int k, float scalar, auto&& ok) {
        if (!tp.plane[k]) return ok(scalar);
        for (size_t e = 0; e < (size_t)tp.trials[k] * npx; e++)
            if (!ok(tp.plane[k][e])) return false;
        return true;
    };
    const bool dead = every_value(NSOF_ACCUM_KEY_VOFF, mo.f.voff, [&](float v) { return !(silent_v < v); }) &&
                      every_value(NSOF_ACCUM_KEY_VON, mo.f.von, [&](float v) { return !(silent_v > v); });
    // no plane but wini with a trial axis: the drives and resistance pairs are one set for all trials
    int drive_trials = 1;
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++)
        if (k != NSOF_ACCUM_KEY_WINI && tp.trials[k] > 1) drive_trials = n_trials;
    const size_t n_drive = (size_t)drive_trials;

    // ---- device memory: the staged stream, the planes, per-array masks / lists / next_ok, the per-trial drives
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    nsof_dev_buf<short> dx, dy;
    nsof_dev_buf<signed char> dp;
    nsof_dev_buf<long long> dbounds, next_ok[2];
    nsof_dev_buf<unsigned> mask[2], list[2], driven[2], count;
    nsof_dev_buf<float> dplane[NSOF_ACCUM_KEY_COUNT], dact, dsil, dres;
    const size_t nev = (size_t)std::max<int64_t>(n_ev, 1);
    int rc = dx.reserve(ctx, nev * 2);
    if (!rc) rc = dy.reserve(ctx, nev * 2);
    if (!rc) rc = dp.reserve(ctx, nev);
    if (!rc) rc = dbounds.reserve(ctx, (size_t)(n_slices + 1) * 8);
    if (!rc) rc = count.reserve(ctx, 4 * sizeof(unsigned));
    for (int i = 0; i < narr && !rc; i++) {
        rc = mask[i].reserve(ctx, npx * sizeof(unsigned));
        if (!rc && dead) rc = list[i].reserve(ctx, nev * sizeof(unsigned));
        if (!rc && dead) rc = driven[i].reserve(ctx, nev * sizeof(unsigned));
        if (!rc && scheme == 2) rc = next_ok[i].reserve(ctx, npx * sizeof(long long));
    }
    if (!rc) rc = dact.reserve(ctx, n_drive * npx * 3 * sizeof(float));
    if (!rc && !dead) rc = dsil.reserve(ctx, n_drive * npx * 3 * sizeof(float));
    if (!rc) rc = dres.reserve(ctx, n_drive * npx * 2 * sizeof(float));
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT && !rc; k++)
        if (tp.plane[k]) rc = dplane[k].reserve(ctx, (size_t)tp.trials[k] * npx * sizeof(float));
    if (rc) return rc;

    hipStream_t st = ctx->stream;
    if (n_ev > 0) {
        NSOF_HIP(ctx, hipMemcpyAsync(dx.p, x + e0, (size_t)n_ev * 2, hipMemcpyHostToDevice, st));
        NSOF_HIP(ctx, hipMemcpyAsync(dy.p, y + e0, (size_t)n_ev * 2, hipMemcpyHostToDevice, st));
        if (p) NSOF_HIP(ctx, hipMemcpyAsync(dp.p, p + e0, (size_t)n_ev, hipMemcpyHostToDevice, st));
    }
    // slice bounds relative to the first staged event; scheme 2: every slice's first timestamp and last + refractory
    std::vector<long long> rel((size_t)n_slices + 1), tfirst((size_t)n_slices, 0), tnext((size_t)n_slices, 0);
    for (int64_t s = 0; s <= n_slices; s++) rel[s] = (long long)(sb[s] - e0);
    if (scheme == 2)
        for (int64_t s = 0; s < n_slices; s++)
            if (sb[s + 1] > sb[s]) {
                tfirst[s] = t[sb[s]];
                tnext[s] = t[sb[s + 1] - 1] + mo.prm.refractory_us;
            }
    NSOF_HIP(ctx, hipMemcpyAsync(dbounds.p, rel.data(), rel.size() * 8, hipMemcpyHostToDevice, st));
    for (int i = 0; i < narr; i++) {
        NSOF_HIP(ctx, hipMemsetAsync(mask[i].p, 0, npx * sizeof(unsigned), st));
        if (scheme == 2) NSOF_HIP(ctx, hipMemsetAsync(next_ok[i].p, 0, npx * sizeof(long long), st));
    }
    NSOF_HIP(ctx, hipMemsetAsync(count.p, 0, 4 * sizeof(unsigned), st));

    const float scal[NSOF_ACCUM_KEY_COUNT] = {mo.f.alphaoff, mo.f.alphaon, mo.f.voff, mo.f.von, mo.f.koff, mo.f.kon, mo.f.son, mo.f.soff,
                                              mo.f.bon, mo.f.boff, mo.f.ron, (float)mo.prm.Roff, mo.wini_f};
    TrialSrc src;
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++) {
        src.plane[k] = nullptr;
        src.stride[k] = 0;
        src.scalar[k] = scal[k];
        if (!tp.plane[k]) continue;
        NSOF_HIP(ctx, hipMemcpyAsync(dplane[k].p, tp.plane[k], (size_t)tp.trials[k] * npx * sizeof(float), hipMemcpyHostToDevice, st));
        src.plane[k] = dplane[k].p;
        src.stride[k] = tp.trials[k] > 1 ? npx : 0;
    }
    src.ron = mo.prm.Ron;
    src.roff = mo.prm.Roff;
    src.dt = mo.f.dt;
    const float v_act = scheme == 1 ? active_v : silent_v + active_v;
    float* const w_arr[2] = {d_w, d_w + T * npx};
    const float2* const res = reinterpret_cast<const float2*>(dres.p);
    const size_t res_stride = drive_trials > 1 ? npx : 0, drive_stride = 3 * res_stride;
    hipLaunchKernelGGL(k_trials_setup, dim3(grid_for(npx), (unsigned)n_trials), dim3(256), 0, st, src, npx, drive_trials, v_act, silent_v,
                       dact.p, dead ? nullptr : dsil.p, reinterpret_cast<float2*>(dres.p), w_arr[0], split ? w_arr[1] : nullptr);
    NSOF_HIP(ctx, hipGetLastError());

    // ---- the groups: up to 32 slices (th.spw with a count threshold), ending right after the next snapshot slice
    const int64_t every = blocks ? snap_every : 0;
    const size_t n_snaps = blocks ? (size_t)((n_slices - 1) / snap_every + 1) : 0;
    const int rows = blocks ? height / memsize : 0, cols = blocks ? width / memsize : 0;
    const int64_t word_slices = theta == 1 ? MAX_GROUP : theta_of(theta).spw;
    const unsigned trial_chunks = (unsigned)((n_trials + TRIAL_CHUNK - 1) / TRIAL_CHUNK);
    int par = 0;   // list counters [parity][array]: a group's resolve zeroes the set the next group's scatter appends to
    size_t snap = 0;
    int64_t s0 = 0;
    while (s0 < n_slices) {
        int64_t g = std::min<int64_t>(n_slices - s0, word_slices);
        if (every > 0) {
            const int64_t to_snap = (s0 % every == 0) ? 1 : (every - s0 % every) + 1;
            if (to_snap < g) g = to_snap;
        }
        const long long ge0 = rel[s0], gn = rel[s0 + g] - ge0;
        unsigned* const cur = count.p + 2 * par;
        unsigned* const nxt = count.p + 2 * (par ^ 1);
        {
            nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
            if (gn > 0)
                with_theta(theta, [&](auto C, auto th) {
                    hipLaunchKernelGGL(k_scatter<decltype(C)::value>, dim3((unsigned)((gn + 255) / 256)), dim3(256), 0, st, dx.p, dy.p, dp.p,
                                       ge0, gn, dbounds.p + s0, (int)g, width, split, mask[0].p, dead ? list[0].p : nullptr, cur,
                                       mask[split].p, dead ? list[split].p : nullptr, cur + 1, (unsigned*)nullptr, th);
                });
            // array i of the group; R: std::true_type for scheme 2, whose kernels take the group's refractory table
            auto update = [&](auto R, const auto& tab, int i) {
                constexpr bool REFR = decltype(R)::value;
                with_theta(theta, [&](auto C, auto th) {
                    constexpr bool COUNT = decltype(C)::value;
                    if constexpr (REFR && COUNT) return;   // refused above
                    else if (dead) {
                        // (a group without events touches no pixel: nothing to launch, the current counter stays zero)
                        if (gn == 0) return;
                        hipLaunchKernelGGL((k_trials_resolve<REFR, COUNT>), dim3(grid_for((size_t)gn, 1024)), dim3(256), 0, st, mask[i].p,
                                           next_ok[i].p, list[i].p, cur + i, tab, driven[i].p, nxt + i, th);
                        hipLaunchKernelGGL(k_trials_update, dim3(grid_for((size_t)gn, 1024), trial_chunks), dim3(256), 0, st, w_arr[i],
                                           list[i].p, cur + i, driven[i].p, dact.p, drive_stride, npx, n_trials, mo.f.dt);
                    } else {
                        hipLaunchKernelGGL((k_trials_update_all<REFR, COUNT>), dim3(grid_for(npx, 8192)), dim3(256), 0, st, w_arr[i],
                                           mask[i].p, next_ok[i].p, npx, (int)g, tab, dact.p, dsil.p, drive_stride, n_trials, mo.f.dt, th);
                    }
                });
            };
            if (scheme == 2) {
                RefrTab tab;
                for (int s = 0; s < 32; s++) {
                    const bool live = s < g && rel[s0 + s + 1] > rel[s0 + s];
                    tab.t_first[s] = live ? tfirst[s0 + s] : 0;
                    tab.t_next[s] = live ? tnext[s0 + s] : 0;
                }
                for (int i = 0; i < narr; i++) update(std::true_type{}, tab, i);
            } else {
                update(std::false_type{}, NoTab{}, 0);
            }
            NSOF_HIP(ctx, hipGetLastError());
        }
        s0 += g;
        if (dead && gn > 0) par ^= 1;
        if (every > 0 && (s0 - 1) % every == 0) {
            for (int i = 0; i < narr; i++)
                hipLaunchKernelGGL(k_trials_block_current, dim3(cols, rows, (unsigned)n_trials), dim3(256), 0, st, w_arr[i], res, res_stride,
                                   npx, width, memsize, cols, snap, n_snaps, v_ds,
                                   d_block_current + (size_t)i * T * n_snaps * (size_t)rows * cols);
            NSOF_HIP(ctx, hipGetLastError());
            snap++;
        }
    }
    const size_t total = (size_t)narr * T * npx;
    hipLaunchKernelGGL(k_trials_resistance, dim3(grid_for(total, 8192)), dim3(256), 0, st, d_w, res, res_stride, npx, n_trials, total,
                       d_resistance);
    NSOF_HIP(ctx, hipGetLastError());
    // the caller's arrays are not retained and the buffers above go with this frame: the run ends here
    NSOF_HIP(ctx, hipStreamSynchronize(st));
    return NSOF_OK;
}
