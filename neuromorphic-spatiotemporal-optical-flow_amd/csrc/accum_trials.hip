// Event-driven accumulator, Monte-Carlo device trials: ONE staged stream drives T arrays whose devices differ (per-pixel,
// per-trial parameter planes) in one run -- nsof_accum_trials_dev.  The float32 arithmetic is accum_update.h's, the one
// the single-array path (accum_kernels.hip) runs: trial t gives, bit for bit, what an accumulator with trial t's planes
// (nsof_accum_set_param_maps) gives on the same stream.
//
// What cannot differ between trials is done once.  Which slices drive which pixel depends on the events alone -- scheme
// 1 compares a pixel's per-slice event count with theta, scheme 2 walks the event times against the pixel's next_ok, and
// neither reads a device parameter -- so per group of up to 32 slices (th.spw with a count threshold), cut at the snapshot
// slices by the single-array path's group_len:
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
// Everything else is the single-array path's own code (accum_model.h, accum_update.h): the check of the plane list, the staged
// stream, the group cuts at the snapshot slices, and -- with the trial as a grid dimension -- k_setup_maps (which also writes the
// initial state here), k_resistance and k_block_min_resistance, the latter taken from the state at the snapshot slices: no
// full-resolution snapshot stack exists.
//
// Cycle-to-cycle write noise (nsof_accum_trials_c2c_dev): every update is scaled by f = max(0, 1 + sigma * xi), xi one
// standard variate per (seed, array, trial, pixel, slice) from a counter generator (c2c_xi: nothing is consumed, so the
// draw does not depend on the grouping, the trial chunk or the kernel form).  The NOISE arms of the two update kernels
// carry it; a call without noise runs the NOISE = false arms, which are the kernels as they were.
//
// The run is an object (nsof_accum_trials): the states, next_ok, the set-up planes and an absolute slice counter stay in HBM
// and nsof_accum_trials_step walks one chunk of the stream at a time -- the groups cut and the snapshots timed by that
// counter, the noise numbered by it, so a chunked run is the one-shot run bit for bit.  The two one-shot entries are create
// (over the caller's d_w), one step, the resistances, destroy.  Per-trial drive voltages reach the set-up kernels as two
// device arrays; k_trials_surface writes the surface frames of all trials in one launch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "accum_c2c.h"
#include "accum_update.h"

namespace {

constexpr int TRIAL_CHUNK = 4;       // trials per thread of k_trials_update
constexpr int MAX_TRIALS = 65535;    // the trial axis is a grid dimension

// ---- cycle-to-cycle write noise ------------------------------------------------------------------------------------------
// (the generator and the variate, philox4x32_10 / c2c_xi / c2c_trial_word: accum_c2c.h, shared with the frame-driven run)
// What a NOISE arm is handed per launch.  branch: per (drive trial, pixel) one byte, bits 0-1 the branch the active drive
// took, bits 2-3 the silent drive's (BR_DEAD: ka = 0, no noise; BR_OFF: V < voff, sigma_off; BR_ON: V > von, sigma_on).
enum { BR_DEAD = 0, BR_OFF = 1, BR_ON = 2 };
struct C2c {
    unsigned k0, k1;
    float sigma_off, sigma_on;
    const unsigned char* branch;
    size_t branch_stride;      // bytes between the planes of consecutive trials (0: one plane for all)
    long long slice0;          // the absolute index of the group's first slice
    unsigned array_word;       // 65536 * array
};
struct NoC2c {};
template <bool NOISE>
using C2cArg = std::conditional_t<NOISE, C2c, NoC2c>;   // no noise passes nothing: the instantiations there always were

__device__ __forceinline__ float sigma_of(const C2c& nz, unsigned br) { return br == BR_OFF ? nz.sigma_off : (br == BR_ON ? nz.sigma_on : 0.f); }

// update_drive with the step scaled by f = max(0, 1 + sigma * xi): a pulse may fail to switch, it never switches backwards.
// Every operation is rounded on its own (-ffp-contract=off).  sigma == 0 -- the dead zone, or a branch without noise -- gives
// f = 1 + 0 = 1 and (g * 1) * dt = g * dt: update_drive's bits, so the draw is skipped.
__device__ __forceinline__ float update_drive_c2c(float w, const Drive& d, float sigma, const C2c& nz, unsigned pix, long long slice,
                                                  unsigned trial_word)
{
    const float g = d.ka * pow_f32(1.f - w * d.s, d.b);
    float f = 1.f;
    if (sigma != 0.f) {
        const float sx = sigma * c2c_xi(nz.k0, nz.k1, pix, (unsigned long long)slice, trial_word);
        const float u = 1.f + sx;
        f = u < 0.f ? 0.f : u;
    }
    const float wn = w + (g * f) * d.dt;
    return wn < 0.f ? 0.f : (wn > 1.f ? 1.f : wn);
}
// replay_driven with each set bit's own slice: the group's first slice plus the slice the bit stands for (a count
// threshold's driven word has one bit per field, in slice order).
__device__ __forceinline__ float replay_driven_c2c(float ww, unsigned m, const Drive& da, float sigma, const C2c& nz, unsigned pix,
                                                   unsigned trial_word)
{
    for (; m; m &= m - 1) ww = update_drive_c2c(ww, da, sigma, nz, pix, nz.slice0 + (__ffs((int)m) - 1), trial_word);
    return ww;
}

// Once per noisy call, per (drive trial = blockIdx.y, pixel): the branches drive_of takes at the two voltages, from the same
// float32 thresholds (a mapped key's value, an unmapped one's scalar) with the same comparisons.  v_act_t, v_sil_t: the
// voltages per trial, as k_setup_maps takes them (nullptr: v_act / v_sil for all).
__global__ __launch_bounds__(256) void k_setup_c2c(MapSrc src, size_t n, float v_act, float v_sil, unsigned char* __restrict__ branch,
                                                    const float* __restrict__ v_act_t, const float* __restrict__ v_sil_t)
{
    const size_t t = blockIdx.y;
    if (v_act_t) {
        v_act = v_act_t[t];
        v_sil = v_sil_t[t];
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        auto get = [&](int k) { return src.plane[k] ? src.plane[k][t * src.stride[k] + i] : src.scalar[k]; };
        const float voff = get(NSOF_ACCUM_KEY_VOFF), von = get(NSOF_ACCUM_KEY_VON);
        auto br = [&](float v) { return v < voff ? (unsigned)BR_OFF : (v > von ? (unsigned)BR_ON : (unsigned)BR_DEAD); };
        branch[t * n + i] = (unsigned char)(br(v_act) | (br(v_sil) << 2));
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
//   NOISE  cycle-to-cycle write noise: one more byte per (trial, listed pixel), the active drive's branch
template <bool NOISE>
__global__ __launch_bounds__(256) void k_trials_update(float* __restrict__ w, const unsigned* __restrict__ list,
                                                        const unsigned* __restrict__ count, const unsigned* __restrict__ driven,
                                                        const float* __restrict__ act, size_t act_stride, size_t npx, int n_trials,
                                                        float dt, C2cArg<NOISE> nz)
{
    const unsigned n = *count;
    const int t0 = blockIdx.y * TRIAL_CHUNK;
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned m = driven[i];
        if (!m) continue;   // no slice of the group drives the pixel: every trial's state stays
        const size_t pix = list[i];
        float ww[TRIAL_CHUNK];
        Drive d[TRIAL_CHUNK];
        [[maybe_unused]] float sg[TRIAL_CHUNK];
#pragma unroll
        for (int k = 0; k < TRIAL_CHUNK; k++)
            if (t0 + k < n_trials) {
                ww[k] = w[(size_t)(t0 + k) * npx + pix];
                d[k] = drive_at(act + (size_t)(t0 + k) * act_stride, pix, dt);
                if constexpr (NOISE) sg[k] = sigma_of(nz, nz.branch[(size_t)(t0 + k) * nz.branch_stride + pix] & 3u);
            }
#pragma unroll
        for (int k = 0; k < TRIAL_CHUNK; k++)
            if (t0 + k < n_trials) {
                if constexpr (NOISE)
                    w[(size_t)(t0 + k) * npx + pix] =
                        replay_driven_c2c(ww[k], m, d[k], sg[k], nz, (unsigned)pix, nz.array_word + (unsigned)(t0 + k));
                else
                    w[(size_t)(t0 + k) * npx + pix] = replay_driven(ww[k], m, d[k]);
            }
    }
}

// The every-pixel form: silent_v outside the dead zone of some pixel of some trial.  One thread per pixel resolves the
// pixel's mask word once and replays all n_sl slices of the group for each trial with that trial's two drives (a pixel whose
// own dead zone holds silent_v carries the no-op drive, ka = 0), as k_update_all does for one mapped array.
//   NOISE  cycle-to-cycle write noise on both drives, each with the sigma of its own branch (a dead-zone drive has none)
template <bool REFR, bool COUNT, bool NOISE>
__global__ __launch_bounds__(256) void k_trials_update_all(float* __restrict__ w, unsigned* __restrict__ mask,
                                                            long long* __restrict__ next_ok, size_t npx, int n_sl, TabArg<REFR> tab,
                                                            const float* __restrict__ act, const float* __restrict__ sil,
                                                            size_t drive_stride, int n_trials, float dt, ThetaArg<COUNT> th,
                                                            C2cArg<NOISE> nz)
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
            if constexpr (NOISE) {
                const unsigned br = nz.branch[(size_t)t * nz.branch_stride + pix];
                const float sa = sigma_of(nz, br & 3u), ss = sigma_of(nz, br >> 2);
                for (int s = 0; s < n_sl; s++) {
                    const bool on = (m >> s) & 1u;
                    ww = update_drive_c2c(ww, on ? pa : ps, on ? sa : ss, nz, (unsigned)pix, nz.slice0 + s, nz.array_word + (unsigned)t);
                }
            } else {
                for (int s = 0; s < n_sl; s++) ww = update_drive(ww, (m >> s) & 1u ? pa : ps);
            }
            w[(size_t)t * npx + pix] = ww;
        }
    }
}

// The surface of one array of every trial (blockIdx.y) as frames: each value formed as k_surface_gray / k_surface_gray_f32
// form it (surface_gray_value; the 8-bit frame truncates, the float frame rounds), the resistance pair of (trial, pixel) read
// through TrialRes where mode 0 needs one.  Write-bound: T * H * W values out, 4 B/px in (mode 0: 12).  A grid-stride loop over
// the pixels (quads) of the trial; consecutive lanes hold consecutive pixels of w and, within a row, of the frame.
//   OutT  uint8_t or float; row_stride / trial_stride in bytes
//   VEC   4: W % 4 == 0 and the frame's address, row stride and trial stride are multiples of 4 * sizeof(OutT) -- a thread
//         loads four states with one 16-byte load and stores their values with one 4- or 16-byte store; 1: pixel by pixel
template <class OutT, int VEC>
__global__ __launch_bounds__(256) void k_trials_surface(const float* __restrict__ w, OutT* __restrict__ out, int W, size_t npx,
                                                         ptrdiff_t row_stride, ptrdiff_t trial_stride, TrialRes res, int mode)
{
    const size_t t = blockIdx.y;
    const float* __restrict__ wt = w + t * npx;
    const float2* __restrict__ rt = res.res + t * res.stride;
    char* const ot = reinterpret_cast<char*>(out) + (ptrdiff_t)t * trial_stride;
    auto value = [&](float ww, size_t pix) { return (OutT)surface_gray_value(ww, res_at(rt, pix, mode), mode); };
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < npx / VEC; q += (size_t)gridDim.x * 256) {
        const size_t pix = q * VEC;                                   // (npx < 2^32: the division is a 32-bit one)
        const unsigned y = (unsigned)pix / (unsigned)W, x = (unsigned)pix % (unsigned)W;
        OutT* const o = reinterpret_cast<OutT*>(ot + (ptrdiff_t)y * row_stride) + x;
        if constexpr (VEC == 4) {
            const float4 v = *reinterpret_cast<const float4*>(wt + pix);
            using Out4 = std::conditional_t<std::is_same_v<OutT, float>, float4, uchar4>;
            Out4 r;
            r.x = value(v.x, pix); r.y = value(v.y, pix + 1); r.z = value(v.z, pix + 2); r.w = value(v.w, pix + 3);
            *reinterpret_cast<Out4*>(o) = r;
        } else {
            *o = value(wt[pix], pix);
        }
    }
}

}  // namespace

// ---- the trial run as an object ------------------------------------------------------------------------------------------
// Everything the one-shot run held in its frame, kept: the states (its own, or the caller's d_w for the one-shot entry), the
// per-array masks / next_ok / lists, the uploaded planes and what the set-up pass made of them, the per-trial voltages, the
// parity of the list counters and the absolute slice counter.
struct nsof_accum_trials {
    nsof_ctx* ctx = nullptr;
    int H = 0, W = 0, scheme = 1, split = 0, narr = 1, theta = 1, n_trials = 1, drive_trials = 1;
    size_t npx = 0;
    Model mo;
    bool dead = true, noise = false;
    nsof_accum_c2c c2c{};
    int64_t snap_every = 0;   // 0: no block currents
    int memsize = 0;
    double v_ds = 1.0;
    float v_act = 0.f, v_sil = 0.f;          // the scalars (read where no voltage is per trial)
    nsof_dev_buf<float> dvact, dvsil;        // [T] each, where a voltage is per trial
    nsof_dev_buf<float> w_own;
    float* w = nullptr;                      // [A][T][npx]: w_own.p, or borrowed
    nsof_dev_buf<long long> next_ok[2];
    nsof_dev_buf<unsigned> mask[2], list[2], driven[2], count;
    nsof_dev_buf<float> dplane[NSOF_ACCUM_KEY_COUNT], dact, dsil, dres;
    nsof_dev_buf<unsigned char> dbranch;
    MapSrc src{};
    StagedStream ev;
    int par = 0;                             // ListCounts' parity, carried from step to step
    int64_t slice_counter = 0;

    float* w_arr(int i) const { return w + (size_t)i * n_trials * npx; }
    TrialRes res() const { return TrialRes{reinterpret_cast<const float2*>(dres.p), drive_trials > 1 ? npx : 0, npx, n_trials}; }
    int rows() const { return memsize ? H / memsize : 0; }
    int cols() const { return memsize ? W / memsize : 0; }
};

namespace {

// What nsof_accum_trials_create takes, and the first chunk of the one-shot entry: its stream is refused before the object
// allocates anything, as that entry always did.
struct TrialsArgs {
    int height, width, scheme, polarity_split;
    const nsof_accum_params* params;
    int theta, n_trials, n_maps;
    const int* keys;
    const float* const* planes;
    const int* plane_trials;
    const nsof_accum_c2c* c2c;
    const float *active_v, *silent_v;
    int n_active, n_silent;
    bool blocks;
    int64_t snap_every;
    int memsize;
    double v_ds;
};
struct Chunk {
    const int16_t *x, *y;
    const int8_t* p;
    const int64_t *t, *sb;
    int64_t n_slices;
    int64_t n_dev = -1;   // >= 0: x, y, p, t are DEVICE arrays of that many events (StagedStream::stage_dev)
};

// the wini planes into the states (k_setup_maps with no drive trial writes nothing else), masks / next_ok / counters zero
int trials_reset(nsof_accum_trials* a, bool setup)
{
    nsof_ctx* ctx = a->ctx;
    hipStream_t st = ctx->stream;
    const size_t npx = a->npx;
    for (int i = 0; i < a->narr; i++) {
        NSOF_HIP(ctx, hipMemsetAsync(a->mask[i].p, 0, npx * sizeof(unsigned), st));
        if (a->scheme == 2) NSOF_HIP(ctx, hipMemsetAsync(a->next_ok[i].p, 0, npx * sizeof(long long), st));
    }
    a->par = 0;
    NSOF_HIP(ctx, (ListCounts{a->count.p}.zero_all(st)));
    hipLaunchKernelGGL(k_setup_maps, dim3(grid_for(npx), (unsigned)a->n_trials), dim3(256), 0, st, a->src, npx, setup ? a->drive_trials : 0,
                       a->v_act, a->v_sil, a->dact.p, a->dead ? nullptr : a->dsil.p, reinterpret_cast<float2*>(a->dres.p), a->w_arr(0),
                       a->split ? a->w_arr(1) : nullptr, (const float*)a->dvact.p, (const float*)a->dvsil.p);
    if (setup && a->noise)
        hipLaunchKernelGGL(k_setup_c2c, dim3(grid_for(npx), (unsigned)a->drive_trials), dim3(256), 0, st, a->src, npx, a->v_act, a->v_sil,
                           a->dbranch.p, (const float*)a->dvact.p, (const float*)a->dvsil.p);
    NSOF_HIP(ctx, hipGetLastError());
    a->slice_counter = 0;
    return NSOF_OK;
}

// borrowed_w: the caller's [A][T][npx] states (the one-shot entry; no second set is allocated).  first: a chunk whose checks
// come before any allocation.
int trials_create(nsof_ctx* ctx, const TrialsArgs& g, float* borrowed_w, const Chunk* first, nsof_accum_trials** out)
{
    // ---- everything that can refuse the call, on the host, before anything is uploaded or launched
    const int height = g.height, width = g.width, scheme = g.scheme, theta = g.theta, n_trials = g.n_trials;
    if (height < 1 || width < 1 || (scheme != 1 && scheme != 2))
        return nsof_set_error(ctx, NSOF_EINVAL, "bad accumulator geometry %dx%d or scheme %d", height, width, scheme);
    if (theta < 1) return nsof_set_error(ctx, NSOF_EINVAL, "event threshold %d: at least 1 event", theta);
    if (scheme == 2 && theta != 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "event threshold %d: scheme 2 has no count threshold (only 1 is accepted)", theta);
    const nsof_accum_c2c* c2c = g.c2c;
    if (c2c) {
        if (!(c2c->sigma_on >= 0.f) || !std::isfinite(c2c->sigma_on))
            return nsof_set_error(ctx, NSOF_EINVAL, "cycle-to-cycle noise: sigma_on = %g is not a finite number >= 0", (double)c2c->sigma_on);
        if (!(c2c->sigma_off >= 0.f) || !std::isfinite(c2c->sigma_off))
            return nsof_set_error(ctx, NSOF_EINVAL, "cycle-to-cycle noise: sigma_off = %g is not a finite number >= 0", (double)c2c->sigma_off);
    }
    const bool noise = c2c && (c2c->sigma_on != 0.f || c2c->sigma_off != 0.f);   // both 0: the noiseless kernels
    Model mo;
    if (int rc = model_of(ctx, g.params, &mo)) return rc;
    PlaneSet<float> tp;
    if (int rc = plane_set_of(ctx, PlaneLabels{"accumulator trials", "trial parameter map"}, mo, height, width, n_trials, g.n_maps, g.keys,
                              g.planes, g.plane_trials, &tp))
        return rc;
    if (g.blocks && (g.snap_every < 1 || g.memsize < 1 || g.memsize > width || g.memsize > height || !(g.v_ds > 0)))
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: block currents need snap_every >= 1 (%lld), 1 <= memsize <= %d (%d), v_ds > 0 (%g)",
                              (long long)g.snap_every, std::min(width, height), g.memsize, g.v_ds);
    if (first && (first->n_slices < 1 || !first->sb)) return nsof_set_error(ctx, NSOF_EINVAL, "bad slice bounds");
    const int64_t n_ev = first ? first->sb[first->n_slices] - first->sb[0] : 0;
    const int split = (scheme == 2 && g.polarity_split) ? 1 : 0, narr = split ? 2 : 1;
    const size_t npx = (size_t)height * width, T = (size_t)n_trials;
    if (npx > 0xFFFFFFFFull) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "sensor too large");
    if (n_trials > MAX_TRIALS || n_ev >= (1ll << 31))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%d trials of %zu pixels, %lld events: too large for one launch", n_trials, npx,
                              (long long)n_ev);
    for (const int n : {g.n_active, g.n_silent})
        if (n != 1 && n != n_trials)
            return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: %d voltages for %d trials (1 or %d)", n, n_trials, n_trials);
    if (!g.active_v || !g.silent_v) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: NULL voltage array");
    const bool v_trials = g.n_active > 1 || g.n_silent > 1;   // (n_trials == 1: one voltage, the scalar path)
    // trial t's two drive voltages; scheme 2 drives with silent_v + active_v, a float32 sum
    std::vector<float> vact(v_trials ? T : 1), vsil(v_trials ? T : 1);
    for (size_t t = 0; t < vact.size(); t++) {
        const float av = g.active_v[g.n_active > 1 ? t : 0];
        vsil[t] = g.silent_v[g.n_silent > 1 ? t : 0];
        vact[t] = scheme == 1 ? av : vsil[t] + av;
    }
    // silent_v inside the dead zone of EVERY pixel of EVERY trial: the touched-pixels form; otherwise the every-pixel form
    const bool dead = v_trials ? silent_in_every_dead_zone(tp, mo.f, vsil.data(), n_trials, npx) : silent_in_every_dead_zone(tp, mo.f, vsil[0], npx);
    // no plane but wini with a trial axis, one voltage pair: the drives and resistance pairs are one set for all trials
    int drive_trials = v_trials ? n_trials : 1;
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++)
        if (k != NSOF_ACCUM_KEY_WINI && tp.trials[k] > 1) drive_trials = n_trials;
    const size_t n_drive = (size_t)drive_trials;
    if (first)
        if (int rc = StagedStream::check(ctx, width, height, scheme, split, first->x, first->y, first->p, first->t, first->sb, first->n_slices))
            return rc;

    // ---- device memory: the states, the planes, per-array masks / next_ok, the per-trial drives (the lists grow with the chunks)
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    nsof_accum_trials* a = new (std::nothrow) nsof_accum_trials();
    if (!a) return nsof_set_error(ctx, NSOF_ENOMEM, "out of host memory");
    a->ctx = ctx; a->H = height; a->W = width; a->scheme = scheme; a->split = split; a->narr = narr; a->theta = theta;
    a->n_trials = n_trials; a->drive_trials = drive_trials; a->npx = npx; a->mo = mo; a->dead = dead; a->noise = noise;
    if (noise) a->c2c = *c2c;
    if (g.blocks) { a->snap_every = g.snap_every; a->memsize = g.memsize; a->v_ds = g.v_ds; }
    a->v_act = vact[0]; a->v_sil = vsil[0];
    int rc = a->count.reserve(ctx, 4 * sizeof(unsigned));
    if (!rc && !borrowed_w) rc = a->w_own.reserve(ctx, (size_t)narr * T * npx * sizeof(float));
    a->w = borrowed_w ? borrowed_w : a->w_own.p;
    for (int i = 0; i < narr && !rc; i++) {
        rc = a->mask[i].reserve(ctx, npx * sizeof(unsigned));
        if (!rc && scheme == 2) rc = a->next_ok[i].reserve(ctx, npx * sizeof(long long));
    }
    if (!rc) rc = a->dact.reserve(ctx, n_drive * npx * 3 * sizeof(float));
    if (!rc && !dead) rc = a->dsil.reserve(ctx, n_drive * npx * 3 * sizeof(float));
    if (!rc) rc = a->dres.reserve(ctx, n_drive * npx * 2 * sizeof(float));
    if (!rc && noise) rc = a->dbranch.reserve(ctx, n_drive * npx);
    if (!rc && v_trials) rc = a->dvact.reserve(ctx, T * sizeof(float));
    if (!rc && v_trials) rc = a->dvsil.reserve(ctx, T * sizeof(float));
    if (!rc) rc = upload_planes(ctx, mo, tp, npx, a->dplane, &a->src);
    auto run = [&]() -> int {
        if (v_trials) {
            NSOF_HIP(ctx, hipMemcpyAsync(a->dvact.p, vact.data(), T * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
            NSOF_HIP(ctx, hipMemcpyAsync(a->dvsil.p, vsil.data(), T * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        }
        if (int r = trials_reset(a, true)) return r;
        // the caller's planes and the voltages above are not retained; the one-shot entry's step synchronises anyway
        if (!first) NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return NSOF_OK;
    };
    if (!rc) rc = run();
    if (rc) { nsof_accum_trials_destroy(a); return rc; }
    *out = a;
    return NSOF_OK;
}

// checked: c is the chunk trials_create has checked already
int trials_step(nsof_accum_trials* a, const Chunk& c, bool checked, double* d_block_current, int64_t* n_snaps_out)
{
    nsof_ctx* ctx = a->ctx;
    const int64_t n_slices = c.n_slices;
    if (n_snaps_out) *n_snaps_out = 0;
    if (n_slices == 0) return NSOF_OK;
    if (n_slices < 0 || !c.sb) return nsof_set_error(ctx, NSOF_EINVAL, "bad slice bounds");
    const int64_t n_ev = c.sb[n_slices] - c.sb[0];
    if (n_ev >= (1ll << 31))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%d trials of %zu pixels, %lld events: too large for one launch", a->n_trials, a->npx,
                              (long long)n_ev);
    const int64_t every = a->snap_every;
    const size_t n_snaps = (size_t)nsof_accum_snaps_between(a->slice_counter, n_slices, every);
    if (n_snaps > 0 && !d_block_current)
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: %zu snapshots fall into the chunk and d_block_current is NULL", n_snaps);
    const int width = a->W, scheme = a->scheme, split = a->split, narr = a->narr, theta = a->theta, n_trials = a->n_trials;
    const size_t npx = a->npx, T = (size_t)n_trials;
    const bool dead = a->dead, noise = a->noise;
    const Model& mo = a->mo;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    StagedStream& ev = a->ev;
    if (int rc = c.n_dev >= 0 ? ev.stage_dev(ctx, width, a->H, scheme, split, mo.prm.refractory_us, c.x, c.y, c.p, c.t, c.n_dev, c.sb, n_slices)
                              : ev.stage(ctx, width, a->H, scheme, split, mo.prm.refractory_us, c.x, c.y, c.p, c.t, c.sb, n_slices, checked))
        return rc;
    if (dead) {
        const size_t nev = (size_t)std::max<int64_t>(n_ev, 1), cap = StagedStream::event_cap(n_ev);
        for (int i = 0; i < narr; i++) {
            if (int rc = a->list[i].reserve(ctx, nev * sizeof(unsigned), cap * sizeof(unsigned))) return rc;
            if (int rc = a->driven[i].reserve(ctx, nev * sizeof(unsigned), cap * sizeof(unsigned))) return rc;
        }
    }
    nsof_dev_buf<unsigned>*const mask = a->mask, *const list = a->list, *const driven = a->driven;
    nsof_dev_buf<long long>* const next_ok = a->next_ok;
    nsof_dev_buf<float>&dact = a->dact, &dsil = a->dsil;

    hipStream_t st = ctx->stream;
    const std::vector<long long>& rel = ev.rel;
    ListCounts cnt{a->count.p, a->par};   // a group's resolve zeroes the set the next group's scatter appends to
    float* const w_arr[2] = {a->w_arr(0), a->w_arr(1)};
    const TrialRes res = a->res();
    const size_t drive_stride = 3 * res.stride;
    C2c nz{};
    if (noise) nz = C2c{(unsigned)a->c2c.seed, (unsigned)(a->c2c.seed >> 32), a->c2c.sigma_off, a->c2c.sigma_on, a->dbranch.p, res.stride, 0, 0};
    // f(std::true_type, the C2c of array i of the group whose first slice has the absolute index s_abs) with noise,
    // f(std::false_type, NoC2c) without
    auto with_noise = [&](int i, int64_t s_abs, auto&& f) {
        if (!noise) return f(std::false_type{}, NoC2c{});
        C2c na = nz;
        na.slice0 = s_abs;
        na.array_word = c2c_trial_word(i, 0);
        f(std::true_type{}, na);
    };

    // ---- the groups: up to 32 slices (th.spw with a count threshold), ending right after the next snapshot slice
    const int rows = a->rows(), cols = a->cols(), memsize = a->memsize;
    const int64_t word_slices = theta == 1 ? MAX_GROUP : theta_of(theta).spw;
    const unsigned trial_chunks = (unsigned)((n_trials + TRIAL_CHUNK - 1) / TRIAL_CHUNK);
    size_t snap = 0;
    int64_t s0 = 0;                     // within the chunk
    int64_t counter = a->slice_counter; // absolute: times the snapshots, cuts the groups, numbers the noise
    while (s0 < n_slices) {
        const int64_t g = group_len(s0, n_slices, word_slices, every, counter);
        const long long ge0 = rel[s0], gn = rel[s0 + g] - ge0;
        unsigned* const cur = cnt.cur();
        unsigned* const nxt = cnt.next();
        {
            nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
            if (gn > 0)
                with_theta(theta, [&](auto C, auto th) {
                    hipLaunchKernelGGL(k_scatter<decltype(C)::value>, dim3((unsigned)((gn + 255) / 256)), dim3(256), 0, st, ev.dx.p, ev.dy.p, ev.dp.p,
                                       ge0, gn, ev.dbounds.p + s0, (int)g, width, split, mask[0].p, dead ? list[0].p : nullptr, cur,
                                       mask[split].p, dead ? list[split].p : nullptr, cur + 1, (unsigned*)nullptr, th);
                });
            // array i of the group; R: std::true_type for scheme 2, whose kernels take the group's refractory table
            auto update = [&](auto R, const auto& tab, int i) {
                constexpr bool REFR = decltype(R)::value;
                with_theta(theta, [&](auto C, auto th) {
                    constexpr bool COUNT = decltype(C)::value;
                    if constexpr (REFR && COUNT) return;   // refused at creation
                    else if (dead) {
                        // (a group without events touches no pixel: nothing to launch, the current counter stays zero)
                        if (gn == 0) return;
                        hipLaunchKernelGGL((k_trials_resolve<REFR, COUNT>), dim3(grid_for((size_t)gn, 1024)), dim3(256), 0, st, mask[i].p,
                                           next_ok[i].p, list[i].p, cur + i, tab, driven[i].p, nxt + i, th);
                        with_noise(i, counter, [&](auto N, auto na) {
                            hipLaunchKernelGGL(k_trials_update<decltype(N)::value>, dim3(grid_for((size_t)gn, 1024), trial_chunks), dim3(256), 0,
                                               st, w_arr[i], list[i].p, cur + i, driven[i].p, dact.p, drive_stride, npx, n_trials, mo.f.dt, na);
                        });
                    } else {
                        with_noise(i, counter, [&](auto N, auto na) {
                            hipLaunchKernelGGL((k_trials_update_all<REFR, COUNT, decltype(N)::value>), dim3(grid_for(npx, 8192)), dim3(256), 0,
                                               st, w_arr[i], mask[i].p, next_ok[i].p, npx, (int)g, tab, dact.p, dsil.p, drive_stride, n_trials,
                                               mo.f.dt, th, na);
                        });
                    }
                });
            };
            if (scheme == 2) {
                const RefrTab tab = refr_tab_of(ev, s0, g);
                for (int i = 0; i < narr; i++) update(std::true_type{}, tab, i);
            } else {
                update(std::false_type{}, NoTab{}, 0);
            }
            NSOF_HIP(ctx, hipGetLastError());
        }
        s0 += g;
        counter += g;
        if (dead && gn > 0) cnt.flip();
        if (snapshot_due(counter, every)) {
            const size_t map = (size_t)rows * cols;   // doubles per (trial, snapshot)
            for (int i = 0; i < narr; i++)
                hipLaunchKernelGGL(k_block_min_resistance<TrialRes>, dim3(cols, rows, (unsigned)n_trials), dim3(256), 0, st, w_arr[i], 1,
                                   width, memsize, cols, res, a->v_ds, d_block_current + ((size_t)i * T * n_snaps + snap) * map, npx,
                                   n_snaps * map);
            NSOF_HIP(ctx, hipGetLastError());
            snap++;
        }
    }
    a->par = cnt.par;
    a->slice_counter = counter;
    if (n_snaps_out) *n_snaps_out = (int64_t)n_snaps;
    return NSOF_OK;
}

int trials_resistance(nsof_accum_trials* a, float* d_out)
{
    const size_t total = (size_t)a->narr * a->n_trials * a->npx;
    hipLaunchKernelGGL(k_resistance<TrialRes>, dim3(grid_for(total, 8192)), dim3(256), 0, a->ctx->stream, a->w, d_out, total, a->res());
    NSOF_HIP(a->ctx, hipGetLastError());
    return NSOF_OK;
}

template <class OutT>
int trials_surface(nsof_accum_trials* a, int which, int mode, OutT* d_out, ptrdiff_t row_stride, ptrdiff_t trial_stride)
{
    nsof_ctx* ctx = a->ctx;
    const ptrdiff_t px = (ptrdiff_t)sizeof(OutT);
    if (!d_out || which < 0 || which >= a->narr || mode < 0 || mode > 1 || row_stride < (ptrdiff_t)a->W * px || row_stride % px ||
        trial_stride % px || reinterpret_cast<uintptr_t>(d_out) % px || trial_stride / a->H < row_stride)
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: surface of array %d, mode %d, row stride %lld, trial stride %lld of a %dx%d sensor",
                              which, mode, (long long)row_stride, (long long)trial_stride, a->H, a->W);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const bool vec = a->W % 4 == 0 && reinterpret_cast<uintptr_t>(d_out) % (4 * px) == 0 && row_stride % (4 * px) == 0 && trial_stride % (4 * px) == 0;
    const dim3 grid(grid_for(a->npx / (vec ? 4 : 1), 1024), (unsigned)a->n_trials);
    if (vec)
        hipLaunchKernelGGL((k_trials_surface<OutT, 4>), grid, dim3(256), 0, ctx->stream, a->w_arr(which), d_out, a->W, a->npx, row_stride,
                           trial_stride, a->res(), mode);
    else
        hipLaunchKernelGGL((k_trials_surface<OutT, 1>), grid, dim3(256), 0, ctx->stream, a->w_arr(which), d_out, a->W, a->npx, row_stride,
                           trial_stride, a->res(), mode);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

}  // namespace

extern "C" void nsof_accum_trials_destroy(nsof_accum_trials* a)
{
    if (!a) return;
    (void)hipSetDevice(a->ctx->device);
    (void)hipStreamSynchronize(a->ctx->stream);
    delete a;
}

extern "C" int nsof_accum_trials_create(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split,
                                        const nsof_accum_params* params, int theta, int n_trials, int n_maps, const int* keys,
                                        const float* const* planes, const int* plane_trials, const nsof_accum_c2c* c2c,
                                        const float* active_v, int n_active, const float* silent_v, int n_silent, int64_t snap_every,
                                        int memsize, double v_ds, nsof_accum_trials** out)
{
    if (!ctx || !out) return NSOF_EINVAL;
    *out = nullptr;
    // (a NULL array or a count that is neither 1 nor n_trials is trials_create's refusal: nothing is read here)
    auto not_finite = [&](const char* name, const float* v, int n) {
        for (int t = 0; v && (n == 1 || n == n_trials) && t < n; t++)
            if (!std::isfinite(v[t]))
                return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: %s of trial %d = %g is not finite", name, t, (double)v[t]);
        return (int)NSOF_OK;
    };
    if (int rc = not_finite("active_v", active_v, n_active)) return rc;
    if (int rc = not_finite("silent_v", silent_v, n_silent)) return rc;
    const TrialsArgs g{height, width, scheme, polarity_split, params, theta, n_trials, n_maps, keys, planes, plane_trials, c2c,
                       active_v, silent_v, n_active, n_silent, memsize != 0, snap_every, memsize, v_ds};
    return trials_create(ctx, g, nullptr, nullptr, out);
}

extern "C" int64_t nsof_accum_snaps_between(int64_t counter, int64_t n_slices, int64_t snap_every)
{
    if (counter < 0 || n_slices < 1 || snap_every < 1) return 0;
    // multiples of snap_every in [counter, counter + n_slices)
    return (counter + n_slices + snap_every - 1) / snap_every - (counter + snap_every - 1) / snap_every;
}

extern "C" int64_t nsof_accum_trials_snaps_in(const nsof_accum_trials* a, int64_t n_slices)
{
    return a ? nsof_accum_snaps_between(a->slice_counter, n_slices, a->snap_every) : 0;
}

extern "C" int nsof_accum_trials_step(nsof_accum_trials* a, const int16_t* x, const int16_t* y, const int8_t* p, const int64_t* t,
                                      const int64_t* sb, int64_t n_slices, double* d_block_current, int64_t* n_snaps)
{
    if (!a) return NSOF_EINVAL;
    if (int rc = trials_step(a, Chunk{x, y, p, t, sb, n_slices}, false, d_block_current, n_snaps)) return rc;
    // the caller's arrays are not retained: the chunk ends here
    NSOF_HIP(a->ctx, hipStreamSynchronize(a->ctx->stream));
    return NSOF_OK;
}

extern "C" int nsof_accum_trials_step_dev(nsof_accum_trials* a, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                                          int64_t n_events, const int64_t* sb, int64_t n_slices, double* d_block_current, int64_t* n_snaps)
{
    if (!a) return NSOF_EINVAL;
    if (n_events < 0) return nsof_set_error(a->ctx, NSOF_EINVAL, "a device stream of %lld events", (long long)n_events);
    if (int rc = trials_step(a, Chunk{d_x, d_y, d_p, d_t, sb, n_slices, n_events}, false, d_block_current, n_snaps)) return rc;
    // the caller's arrays are not retained: the chunk ends here
    NSOF_HIP(a->ctx, hipStreamSynchronize(a->ctx->stream));
    return NSOF_OK;
}

extern "C" int nsof_accum_trials_w_dev(nsof_accum_trials* a, float* d_out)
{
    if (!a || !d_out) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    NSOF_HIP(ctx, hipMemcpyAsync(d_out, a->w, (size_t)a->narr * a->n_trials * a->npx * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return NSOF_OK;
}

extern "C" int nsof_accum_trials_resistance_dev(nsof_accum_trials* a, float* d_out)
{
    if (!a || !d_out) return NSOF_EINVAL;
    NSOF_HIP(a->ctx, hipSetDevice(a->ctx->device));
    return trials_resistance(a, d_out);
}

extern "C" int nsof_accum_trials_block_current_dev(nsof_accum_trials* a, double* d_out)
{
    if (!a || !d_out) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (!a->memsize) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: block currents need a memsize at creation");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const int rows = a->rows(), cols = a->cols();
    const size_t map = (size_t)rows * cols;
    for (int i = 0; i < a->narr; i++)
        hipLaunchKernelGGL(k_block_min_resistance<TrialRes>, dim3(cols, rows, (unsigned)a->n_trials), dim3(256), 0, ctx->stream, a->w_arr(i), 1,
                           a->W, a->memsize, cols, a->res(), a->v_ds, d_out + (size_t)i * a->n_trials * map, a->npx, map);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_accum_trials_surface_u8_dev(nsof_accum_trials* a, int which, int mode, uint8_t* d_out, ptrdiff_t row_stride,
                                                ptrdiff_t trial_stride)
{
    return a ? trials_surface<uint8_t>(a, which, mode, d_out, row_stride, trial_stride) : NSOF_EINVAL;
}

extern "C" int nsof_accum_trials_surface_f32_dev(nsof_accum_trials* a, int which, int mode, float* d_out, ptrdiff_t row_stride_bytes,
                                                 ptrdiff_t trial_stride_bytes)
{
    return a ? trials_surface<float>(a, which, mode, d_out, row_stride_bytes, trial_stride_bytes) : NSOF_EINVAL;
}

extern "C" int nsof_accum_trials_read_state(nsof_accum_trials* a, float* w_out, int64_t* next_ok_out, int64_t* slice_counter)
{
    if (!a) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (slice_counter) *slice_counter = a->slice_counter;
    if (!w_out && !next_ok_out) return NSOF_OK;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    if (w_out) NSOF_HIP(ctx, hipMemcpyAsync(w_out, a->w, (size_t)a->narr * a->n_trials * a->npx * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    for (int i = 0; next_ok_out && i < a->narr; i++) {
        if (a->scheme == 2)
            NSOF_HIP(ctx, hipMemcpyAsync(next_ok_out + (size_t)i * a->npx, a->next_ok[i].p, a->npx * 8, hipMemcpyDeviceToHost, ctx->stream));
        else
            memset(next_ok_out + (size_t)i * a->npx, 0, a->npx * 8);
    }
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NSOF_OK;
}

extern "C" int nsof_accum_trials_write_state(nsof_accum_trials* a, const float* w_in, int64_t n_w_planes, const int64_t* next_ok_in,
                                             int64_t n_next_ok_planes, int64_t slice_counter)
{
    if (!a) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (!w_in || n_w_planes != (int64_t)a->narr * a->n_trials)
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: a state of %lld planes, the object holds %d arrays of %d trials",
                              (long long)n_w_planes, a->narr, a->n_trials);
    if (next_ok_in && n_next_ok_planes != a->narr)
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: %lld next_ok planes, the object holds %d arrays", (long long)n_next_ok_planes,
                              a->narr);
    if (slice_counter < 0) return nsof_set_error(ctx, NSOF_EINVAL, "negative slice counter");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    NSOF_HIP(ctx, hipMemcpyAsync(a->w, w_in, (size_t)n_w_planes * a->npx * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    for (int i = 0; a->scheme == 2 && i < a->narr; i++) {
        if (next_ok_in)
            NSOF_HIP(ctx, hipMemcpyAsync(a->next_ok[i].p, next_ok_in + (size_t)i * a->npx, a->npx * 8, hipMemcpyHostToDevice, ctx->stream));
        else
            NSOF_HIP(ctx, hipMemsetAsync(a->next_ok[i].p, 0, a->npx * 8, ctx->stream));
    }
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    a->slice_counter = slice_counter;
    return NSOF_OK;
}

extern "C" int nsof_accum_trials_reset(nsof_accum_trials* a)
{
    if (!a) return NSOF_EINVAL;
    NSOF_HIP(a->ctx, hipSetDevice(a->ctx->device));
    return trials_reset(a, false);
}

extern "C" void nsof_accum_c2c_noise(uint64_t seed, int array, int trial, uint32_t pixel, int64_t slice, int64_t n_slices, float* out)
{
    for (int64_t i = 0; i < n_slices; i++)
        out[i] = c2c_xi((unsigned)seed, (unsigned)(seed >> 32), pixel, (unsigned long long)slice + (unsigned long long)i,
                        c2c_trial_word(array, trial));
}

extern "C" int nsof_accum_trials_dev(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v,
                                     float silent_v, const nsof_accum_params* params, int theta, const int16_t* x, const int16_t* y,
                                     const int8_t* p, const int64_t* t, const int64_t* sb, int64_t n_slices, int64_t snap_every,
                                     int memsize, double v_ds, int n_trials, int n_maps, const int* keys, const float* const* planes,
                                     const int* plane_trials, float* d_w, float* d_resistance, double* d_block_current)
{
    return nsof_accum_trials_c2c_dev(ctx, height, width, scheme, polarity_split, active_v, silent_v, params, theta, x, y, p, t, sb, n_slices,
                                     snap_every, memsize, v_ds, n_trials, n_maps, keys, planes, plane_trials, d_w, d_resistance,
                                     d_block_current, nullptr);
}

extern "C" int nsof_accum_trials_c2c_dev(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v,
                                         float silent_v, const nsof_accum_params* params, int theta, const int16_t* x, const int16_t* y,
                                         const int8_t* p, const int64_t* t, const int64_t* sb, int64_t n_slices, int64_t snap_every,
                                         int memsize, double v_ds, int n_trials, int n_maps, const int* keys,
                                         const float* const* planes, const int* plane_trials, float* d_w, float* d_resistance,
                                         double* d_block_current, const nsof_accum_c2c* c2c)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_w || !d_resistance) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: NULL output");
    // The object over the caller's d_w, the whole stream as its one chunk (checked with everything else that can refuse the
    // call, before anything is allocated, uploaded or launched), the resistances of the final states.
    const TrialsArgs g{height, width, scheme, polarity_split, params, theta, n_trials, n_maps, keys, planes, plane_trials, c2c,
                       &active_v, &silent_v, 1, 1, d_block_current != nullptr, snap_every, memsize, v_ds};
    const Chunk all{x, y, p, t, sb, n_slices};
    nsof_accum_trials* a = nullptr;
    if (int rc = trials_create(ctx, g, d_w, &all, &a)) return rc;
    int rc = trials_step(a, all, true, d_block_current, nullptr);
    if (!rc) rc = trials_resistance(a, d_resistance);
    // the caller's arrays are not retained and the object goes with this frame: the run ends here
    auto finish = [&]() -> int {
        NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return NSOF_OK;
    };
    if (!rc) rc = finish();
    nsof_accum_trials_destroy(a);
    return rc;
}
