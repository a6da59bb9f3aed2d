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
#include <algorithm>
#include <cmath>
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
// float32 thresholds (a mapped key's value, an unmapped one's scalar) with the same comparisons.
__global__ __launch_bounds__(256) void k_setup_c2c(MapSrc src, size_t n, float v_act, float v_sil, unsigned char* __restrict__ branch)
{
    const size_t t = blockIdx.y;
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

}  // namespace

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
    // ---- everything that can refuse the call, on the host, before anything is uploaded or launched (the stream's own checks
    // are StagedStream::stage's, below, ahead of its uploads)
    if (!d_w || !d_resistance) return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: NULL output");
    if (height < 1 || width < 1 || (scheme != 1 && scheme != 2))
        return nsof_set_error(ctx, NSOF_EINVAL, "bad accumulator geometry %dx%d or scheme %d", height, width, scheme);
    if (theta < 1) return nsof_set_error(ctx, NSOF_EINVAL, "event threshold %d: at least 1 event", theta);
    if (scheme == 2 && theta != 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "event threshold %d: scheme 2 has no count threshold (only 1 is accepted)", theta);
    if (c2c) {
        if (!(c2c->sigma_on >= 0.f) || !std::isfinite(c2c->sigma_on))
            return nsof_set_error(ctx, NSOF_EINVAL, "cycle-to-cycle noise: sigma_on = %g is not a finite number >= 0", (double)c2c->sigma_on);
        if (!(c2c->sigma_off >= 0.f) || !std::isfinite(c2c->sigma_off))
            return nsof_set_error(ctx, NSOF_EINVAL, "cycle-to-cycle noise: sigma_off = %g is not a finite number >= 0", (double)c2c->sigma_off);
    }
    const bool noise = c2c && (c2c->sigma_on != 0.f || c2c->sigma_off != 0.f);   // both 0: the noiseless kernels
    Model mo;
    if (int rc = model_of(ctx, params, &mo)) return rc;
    PlaneSet<float> tp;
    if (int rc = plane_set_of(ctx, PlaneLabels{"accumulator trials", "trial parameter map"}, mo, height, width, n_trials, n_maps, keys,
                              planes, plane_trials, &tp))
        return rc;
    const bool blocks = d_block_current != nullptr;
    if (blocks && (snap_every < 1 || memsize < 1 || memsize > width || memsize > height || !(v_ds > 0)))
        return nsof_set_error(ctx, NSOF_EINVAL, "accumulator trials: block currents need snap_every >= 1 (%lld), 1 <= memsize <= %d (%d), v_ds > 0 (%g)",
                              (long long)snap_every, std::min(width, height), memsize, v_ds);
    if (n_slices < 1 || !sb) return nsof_set_error(ctx, NSOF_EINVAL, "bad slice bounds");
    const int64_t n_ev = sb[n_slices] - sb[0];
    const int split = (scheme == 2 && polarity_split) ? 1 : 0, narr = split ? 2 : 1;
    const size_t npx = (size_t)height * width, T = (size_t)n_trials;
    if (npx > 0xFFFFFFFFull) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "sensor too large");
    if (n_trials > MAX_TRIALS || n_ev >= (1ll << 31))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%d trials of %zu pixels, %lld events: too large for one launch", n_trials, npx,
                              (long long)n_ev);
    // silent_v inside the dead zone of EVERY pixel of EVERY trial: the touched-pixels form; otherwise the every-pixel form
    const bool dead = silent_in_every_dead_zone(tp, mo.f, silent_v, npx);
    // no plane but wini with a trial axis: the drives and resistance pairs are one set for all trials
    int drive_trials = 1;
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++)
        if (k != NSOF_ACCUM_KEY_WINI && tp.trials[k] > 1) drive_trials = n_trials;
    const size_t n_drive = (size_t)drive_trials;

    // ---- device memory: the staged stream (refusing a bad one), the planes, per-array masks / lists / next_ok, the per-trial drives
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    StagedStream ev;
    if (int rc = ev.stage(ctx, width, height, scheme, split, mo.prm.refractory_us, x, y, p, t, sb, n_slices)) return rc;
    nsof_dev_buf<long long> next_ok[2];
    nsof_dev_buf<unsigned> mask[2], list[2], driven[2], count;
    nsof_dev_buf<float> dplane[NSOF_ACCUM_KEY_COUNT], dact, dsil, dres;
    nsof_dev_buf<unsigned char> dbranch;
    const size_t nev = (size_t)std::max<int64_t>(n_ev, 1);
    int rc = count.reserve(ctx, 4 * sizeof(unsigned));
    for (int i = 0; i < narr && !rc; i++) {
        rc = mask[i].reserve(ctx, npx * sizeof(unsigned));
        if (!rc && dead) rc = list[i].reserve(ctx, nev * sizeof(unsigned));
        if (!rc && dead) rc = driven[i].reserve(ctx, nev * sizeof(unsigned));
        if (!rc && scheme == 2) rc = next_ok[i].reserve(ctx, npx * sizeof(long long));
    }
    if (!rc) rc = dact.reserve(ctx, n_drive * npx * 3 * sizeof(float));
    if (!rc && !dead) rc = dsil.reserve(ctx, n_drive * npx * 3 * sizeof(float));
    if (!rc) rc = dres.reserve(ctx, n_drive * npx * 2 * sizeof(float));
    if (!rc && noise) rc = dbranch.reserve(ctx, n_drive * npx);
    MapSrc src;
    if (!rc) rc = upload_planes(ctx, mo, tp, npx, dplane, &src);
    if (rc) return rc;

    hipStream_t st = ctx->stream;
    const std::vector<long long>& rel = ev.rel;
    for (int i = 0; i < narr; i++) {
        NSOF_HIP(ctx, hipMemsetAsync(mask[i].p, 0, npx * sizeof(unsigned), st));
        if (scheme == 2) NSOF_HIP(ctx, hipMemsetAsync(next_ok[i].p, 0, npx * sizeof(long long), st));
    }
    ListCounts cnt{count.p};   // a group's resolve zeroes the set the next group's scatter appends to
    NSOF_HIP(ctx, cnt.zero_all(st));
    const float v_act = scheme == 1 ? active_v : silent_v + active_v;
    float* const w_arr[2] = {d_w, d_w + T * npx};
    const TrialRes res{reinterpret_cast<const float2*>(dres.p), drive_trials > 1 ? npx : 0, npx, n_trials};
    const size_t drive_stride = 3 * res.stride;
    hipLaunchKernelGGL(k_setup_maps, dim3(grid_for(npx), (unsigned)n_trials), dim3(256), 0, st, src, npx, drive_trials, v_act, silent_v,
                       dact.p, dead ? nullptr : dsil.p, reinterpret_cast<float2*>(dres.p), w_arr[0], split ? w_arr[1] : nullptr);
    C2c nz{};
    if (noise) {
        nz = C2c{(unsigned)c2c->seed, (unsigned)(c2c->seed >> 32), c2c->sigma_off, c2c->sigma_on, dbranch.p, res.stride, 0, 0};
        hipLaunchKernelGGL(k_setup_c2c, dim3(grid_for(npx), (unsigned)drive_trials), dim3(256), 0, st, src, npx, v_act, silent_v, dbranch.p);
    }
    NSOF_HIP(ctx, hipGetLastError());
    // f(std::true_type, the C2c of array i of the group from slice s0) with noise, f(std::false_type, NoC2c) without
    auto with_noise = [&](int i, int64_t s0, auto&& f) {
        if (!noise) return f(std::false_type{}, NoC2c{});
        C2c a = nz;
        a.slice0 = s0;
        a.array_word = c2c_trial_word(i, 0);
        f(std::true_type{}, a);
    };

    // ---- the groups: up to 32 slices (th.spw with a count threshold), ending right after the next snapshot slice
    const int64_t every = blocks ? snap_every : 0;
    const size_t n_snaps = blocks ? (size_t)((n_slices - 1) / snap_every + 1) : 0;
    const int rows = blocks ? height / memsize : 0, cols = blocks ? width / memsize : 0;
    const int64_t word_slices = theta == 1 ? MAX_GROUP : theta_of(theta).spw;
    const unsigned trial_chunks = (unsigned)((n_trials + TRIAL_CHUNK - 1) / TRIAL_CHUNK);
    size_t snap = 0;
    int64_t s0 = 0;   // also the slice counter: the run starts at a fresh array
    while (s0 < n_slices) {
        const int64_t g = group_len(s0, n_slices, word_slices, every, s0);
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
                    if constexpr (REFR && COUNT) return;   // refused above
                    else if (dead) {
                        // (a group without events touches no pixel: nothing to launch, the current counter stays zero)
                        if (gn == 0) return;
                        hipLaunchKernelGGL((k_trials_resolve<REFR, COUNT>), dim3(grid_for((size_t)gn, 1024)), dim3(256), 0, st, mask[i].p,
                                           next_ok[i].p, list[i].p, cur + i, tab, driven[i].p, nxt + i, th);
                        with_noise(i, s0, [&](auto N, auto na) {
                            hipLaunchKernelGGL(k_trials_update<decltype(N)::value>, dim3(grid_for((size_t)gn, 1024), trial_chunks), dim3(256), 0,
                                               st, w_arr[i], list[i].p, cur + i, driven[i].p, dact.p, drive_stride, npx, n_trials, mo.f.dt, na);
                        });
                    } else {
                        with_noise(i, s0, [&](auto N, auto na) {
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
        if (dead && gn > 0) cnt.flip();
        if (snapshot_due(s0, every)) {
            const size_t map = (size_t)rows * cols;   // doubles per (trial, snapshot)
            for (int i = 0; i < narr; i++)
                hipLaunchKernelGGL(k_block_min_resistance<TrialRes>, dim3(cols, rows, (unsigned)n_trials), dim3(256), 0, st, w_arr[i], 1,
                                   width, memsize, cols, res, v_ds, d_block_current + ((size_t)i * T * n_snaps + snap) * map, npx,
                                   n_snaps * map);
            NSOF_HIP(ctx, hipGetLastError());
            snap++;
        }
    }
    const size_t total = (size_t)narr * T * npx;
    hipLaunchKernelGGL(k_resistance<TrialRes>, dim3(grid_for(total, 8192)), dim3(256), 0, st, d_w, d_resistance, total, res);
    NSOF_HIP(ctx, hipGetLastError());
    // the caller's arrays are not retained and the buffers above go with this frame: the run ends here
    NSOF_HIP(ctx, hipStreamSynchronize(st));
    return NSOF_OK;
}
