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
#include <algorithm>
#include <cmath>
#include <vector>

#include "accum_update.h"

namespace {

constexpr int TRIAL_CHUNK = 4;       // trials per thread of k_trials_update
constexpr int MAX_TRIALS = 65535;    // the trial axis is a grid dimension

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

}  // namespace

extern "C" int nsof_accum_trials_dev(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v,
                                     float silent_v, const nsof_accum_params* params, int theta, const int16_t* x, const int16_t* y,
                                     const int8_t* p, const int64_t* t, const int64_t* sb, int64_t n_slices, int64_t snap_every,
                                     int memsize, double v_ds, int n_trials, int n_maps, const int* keys, const float* const* planes,
                                     const int* plane_trials, float* d_w, float* d_resistance, double* d_block_current)
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
    NSOF_HIP(ctx, hipGetLastError());

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
                        hipLaunchKernelGGL(k_trials_update, dim3(grid_for((size_t)gn, 1024), trial_chunks), dim3(256), 0, st, w_arr[i],
                                           list[i].p, cur + i, driven[i].p, dact.p, drive_stride, npx, n_trials, mo.f.dt);
                    } else {
                        hipLaunchKernelGGL((k_trials_update_all<REFR, COUNT>), dim3(grid_for(npx, 8192)), dim3(256), 0, st, w_arr[i],
                                           mask[i].p, next_ok[i].p, npx, (int)g, tab, dact.p, dsil.p, drive_stride, n_trials, mo.f.dt, th);
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
