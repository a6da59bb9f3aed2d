// Synaptic accumulator ("memristor array"), event-driven, float32: HIP kernels + host driver for gfx950.  (The float64
// frame-driven run is accum_frames.hip; the device model both take is accum_model.h.  The update arithmetic, the scatter, the
// count threshold and the refractory walk are accum_update.h, shared with the trial run of accum_trials.hip.)
//
// Replaces /root/reference/eventsim/event_mem_sim.py: update_state (:40-57),
// resistance_exp (:60-63) and the slice loop of simulate (:164-286).
//
// Design (MI355X-first, not a translation of the per-slice NumPy passes):
//  * Pixels are independent and time is serial per pixel, so up to 32 consecutive slices are
//    fused into ONE pass over the state: a scatter kernel ORs "pixel active in slice s" bits
//    into a u32 mask per pixel; the update kernel reads w once, replays the 32 slices in
//    registers and writes w once.  HBM traffic drops from 8 B/px/slice to <= 16/S B/px/slice.
//  * When silent_v lies in the device's dead zone [voff, von] (the default, 0 V) an inactive
//    pixel is a bit-exact no-op (dw/dt = 0, clip is the identity on [0,1]); then only the
//    pixels touched by events are visited (compacted list built by the scatter kernel).
//  * Scheme 2's refractory rule couples consecutive slices through next_ok, but per pixel only:
//    one scatter per group as in scheme 1, the eligibility walk inside the fused update (RefrTab).
//  * The device model (PARAMS, DT, REFRACTORY_US of the reference) is an argument of the accumulator (nsof_accum_params):
//    float32 fields by value in the kernel arguments, the fitted device of the paper as a compile-time instantiation of
//    the hot kernels (DevF, fitted_f: accum_model.h).  Per-pixel parameter maps (nsof_accum_set_param_maps) are a third kind: one
//    set-up kernel writes every pixel's drives and resistance pair, the hot kernels load them per driven pixel (MapF).
//  * pow/exp go through double precision so that the float32 result is the correctly
//    rounded one: equal to it on every state in [0, 1] outside the ~3e-7 of inputs that lie
//    within 2^-43 of a rounding midpoint, and on those too as measured (tests/test_accum_cr_gpu.py;
//    the reference's NumPy uses SIMD pow/exp that are themselves 1-4 ulp off libm, hence the
//    tolerances against its goldens in tests/test_accum_gpu.py).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "accum_update.h"

namespace {

struct NoModel {};
// KIND of the hot kernels (DevF, fitted_f, MapF: accum_model.h): the fitted device as compile-time constants / one device in the kernel arguments / per-pixel planes.
// (int constants, not an unnamed enum: ModelArg<KIND> is part of every hot kernel's signature, and an unnamed type in a mangled
// name is numbered differently by the host and the device pass -- the host would register a name the code object lacks)
constexpr int MK_FITTED = 0, MK_UNIFORM = 1, MK_MAPPED = 2;
template <int KIND>
using ModelArg = std::conditional_t<KIND == MK_FITTED, NoModel, std::conditional_t<KIND == MK_UNIFORM, DevF, MapF>>;
template <int KIND>
using KindTag = std::integral_constant<int, KIND>;
__device__ __forceinline__ DevF model_arg(const DevF& p) { return p; }
__device__ __forceinline__ DevF model_arg(NoModel) { return fitted_f(); }
__device__ __forceinline__ DevF model_arg(const MapF& m)   // dt is all the pixels share
{
    DevF p{};
    p.dt = m.dt;
    return p;
}
__global__ __launch_bounds__(256) void k_update_state(const float* __restrict__ w, const float* __restrict__ V,
                                                       float* __restrict__ out, size_t n, DevF p)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        out[i] = update_one(w[i], V[i], p);
}

__global__ __launch_bounds__(256) void k_fill(float* __restrict__ p, size_t n, float v)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = v;
}

// (surface_gray_value / surface_gray_one: accum_update.h, shared with the trial run's surface kernel)
// Where the fused dense update leaves the frame of the state it has just written (out == nullptr: nowhere).
struct SurfOut {
    uint8_t* out;
    long long stride;
    int W;
    int mode;
};

// Fused state update over the touched pixels only (silent_v inside the dead zone): walks the compact list, claims each
// pixel's mask, replays its driven slices and stores w.
//   REFR   scheme 2: the mask holds event bits; refractory_walk turns them into driven bits first
//   MaskT  the mask word: 32 bits (groups of up to 32 slices), 64 bits (copy + patch: intervals of up to 64 slices)
//   FRAME  the pixel's byte of the frame `so` is overwritten as well (copy + patch)
//   KIND   the model (ModelArg): MK_FITTED the fitted device as compile-time constants, MK_UNIFORM one device in the arguments,
//          MK_MAPPED every pixel its own (its active drive, and for the frame its resistance pair, loaded per listed pixel)
//   COUNT  scheme 1 with theta > 1: the word holds counter fields; driven_bits turns them into driven bits first
template <bool REFR, class MaskT, bool FRAME, int KIND, bool COUNT>
__global__ __launch_bounds__(256) void k_update_list(float* __restrict__ w, MaskT* __restrict__ mask,
                                                      long long* __restrict__ next_ok, const unsigned* __restrict__ list,
                                                      const unsigned* __restrict__ count, TabArg<REFR> tab, float v_act,
                                                      unsigned* zero_next, SurfOut so, ModelArg<KIND> model, ThetaArg<COUNT> th)
{
    const DevF p = model_arg(model);
    __shared__ long long tf[REFR ? 32 : 1], tn[REFR ? 32 : 1];
    if constexpr (REFR) {
        if (threadIdx.x < 32) { tf[threadIdx.x] = tab.t_first[threadIdx.x]; tn[threadIdx.x] = tab.t_next[threadIdx.x]; }
        __syncthreads();
    }
    const unsigned n = *count;
    if (zero_next && blockIdx.x == 0 && threadIdx.x == 0) *zero_next = 0;   // the NEXT group's list counter (other parity)
    const Drive da = drive_of(v_act, p);
    for (unsigned i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned pix = list[i];
        MaskT m = mask[pix];
        mask[pix] = 0;
        if constexpr (COUNT) {
            m = driven_bits(m, th);
            if (!m) continue;   // no cell of the pixel reached theta: state and frame byte stay
        }
        if constexpr (REFR) {
            long long ok = next_ok[pix];
            m = refractory_walk(m, ok, tf, tn);
            if (!m) continue;
            next_ok[pix] = ok;
        }
        float ww;
        if constexpr (KIND == MK_MAPPED) ww = replay_driven(w[pix], m, drive_at(model.act, pix, p.dt));
        else ww = replay_driven(w[pix], m, da);
        w[pix] = ww;
        if constexpr (FRAME) {
            const unsigned yy = pix / (unsigned)so.W, xx = pix - yy * (unsigned)so.W;
            if constexpr (KIND == MK_MAPPED) so.out[(long long)yy * so.stride + xx] = surface_gray_one(ww, res_at(model.res, pix, so.mode), so.mode);
            else so.out[(long long)yy * so.stride + xx] = surface_gray_one(ww, p, so.mode);
        }
    }
}

// Fused state update over every pixel (silent_v outside the dead zone, or forced dense).
// 4 pixels per thread: one 16-B load/store of w and of the mask per lane.
//   REFR      scheme 2: refractory_walk on every touched pixel, as in k_update_list; it has neither a second mask word nor
//             a fused frame.  Scheme 1: m = slices 0..31 of the group, mh = slices 32..63 (groups of up to 64 slices: one
//             pass over the array where a frame interval of 33 slices took two), and the frame of the new state in `so`.
//   SIL_NOOP  silent_v lies in the dead zone [voff, von], where update_state leaves w bit-for-bit unchanged (dw = 0, w
//             already inside [0,1]), so only the slices whose bit is set are replayed (in slice order) -- the pass is then
//             bound by its one read and one write of the state instead of by 32 no-op evaluations per pixel.
//   COUNT     scheme 1 with theta > 1: both words hold counter fields, th.spw slices each; driven_bits first
//   KIND      MK_MAPPED: a pixel loads its own drives -- the active one only, and only if it is driven, under SIL_NOOP (which
//             then means: silent_v in the dead zone of EVERY pixel); both otherwise, a pixel whose own dead zone holds
//             silent_v carrying the no-op drive (ka = 0) -- and its resistance pair for a mode-0 frame
template <bool REFR, bool SIL_NOOP, int KIND, bool COUNT>
__global__ __launch_bounds__(256) void k_update_all(float* __restrict__ w, unsigned* __restrict__ mask,
                                                     unsigned* __restrict__ mask_hi, long long* __restrict__ next_ok, size_t n4,
                                                     size_t n, int n_sl, TabArg<REFR> tab, float v_act, float v_sil, SurfOut so,
                                                     ModelArg<KIND> model, ThetaArg<COUNT> th)
{
    const DevF p = model_arg(model);
    __shared__ long long tf[REFR ? 32 : 1], tn[REFR ? 32 : 1];
    if constexpr (REFR) {
        if (threadIdx.x < 32) { tf[threadIdx.x] = tab.t_first[threadIdx.x]; tn[threadIdx.x] = tab.t_next[threadIdx.x]; }
        __syncthreads();
        mask_hi = nullptr;   // known at compile time: the scheme-2 instantiations carry no code for either
        so.out = nullptr;
    }
    const Drive da = drive_of(v_act, p), ds = drive_of(v_sil, p);
    int lo_sl = 32;   // slices of the first mask word
    if constexpr (COUNT) lo_sl = th.spw;
    auto one = [&](float ww, unsigned m, unsigned mh, size_t pix) {
        if constexpr (COUNT) {
            m = driven_bits(m, th);
            mh = driven_bits(mh, th);
        }
        if constexpr (REFR) {
            if (m) {
                long long ok = next_ok[pix];
                m = refractory_walk(m, ok, tf, tn);
                if (m) next_ok[pix] = ok;
            }
        }
        if constexpr (KIND == MK_MAPPED) {
            if (SIL_NOOP) {
                if (!(m | mh)) return ww;
                const Drive pa = drive_at(model.act, pix, p.dt);
                return replay_driven(replay_driven(ww, m, pa), mh, pa);
            }
            const Drive pa = drive_at(model.act, pix, p.dt), ps = drive_at(model.sil, pix, p.dt);
            for (int s = 0; s < n_sl; s++) {
                const bool act = (REFR || s < lo_sl) ? (m >> s) & 1u : (mh >> (s - lo_sl)) & 1u;
                ww = update_drive(ww, act ? pa : ps);
            }
            return ww;
        } else {
        if (SIL_NOOP) return replay_driven(replay_driven(ww, m, da), mh, da);
        for (int s = 0; s < n_sl; s++) {
            const bool act = (REFR || s < lo_sl) ? (m >> s) & 1u : (mh >> (s - lo_sl)) & 1u;
            Drive d;
            d.dt = da.dt;
            d.ka = act ? da.ka : ds.ka;
            d.s = act ? da.s : ds.s;
            d.b = act ? da.b : ds.b;
            ww = update_drive(ww, d);
        }
        return ww;
        }
    };
    // the byte of the new state's frame at pixel pix
    auto gray = [&](float v, size_t pix) {
        if constexpr (KIND == MK_MAPPED) return surface_gray_one(v, res_at(model.res, pix, so.mode), so.mode);
        else return surface_gray_one(v, p, so.mode);
    };
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        if (4 * i + 3 < n) {
            float4 ww = reinterpret_cast<float4*>(w)[i];
            const uint4 mm = reinterpret_cast<uint4*>(mask)[i];
            const bool any = (mm.x | mm.y | mm.z | mm.w) != 0;
            // nothing driven: w unchanged bit for bit.  Scheme 1 stores every quad: its fused frame needs every pixel.
            if (REFR && SIL_NOOP && !any) continue;
            if (any) reinterpret_cast<uint4*>(mask)[i] = make_uint4(0, 0, 0, 0);
            uint4 mh = make_uint4(0, 0, 0, 0);
            if (mask_hi) {
                mh = reinterpret_cast<uint4*>(mask_hi)[i];
                if (mh.x | mh.y | mh.z | mh.w) reinterpret_cast<uint4*>(mask_hi)[i] = make_uint4(0, 0, 0, 0);
            }
            ww.x = one(ww.x, mm.x, mh.x, 4 * i);
            ww.y = one(ww.y, mm.y, mh.y, 4 * i + 1);
            ww.z = one(ww.z, mm.z, mh.z, 4 * i + 2);
            ww.w = one(ww.w, mm.w, mh.w, 4 * i + 3);
            reinterpret_cast<float4*>(w)[i] = ww;
            if (so.out) {   // the frame of the new state: saves the separate surface pass (4 B/px read again + a launch)
                const size_t px = 4 * i;
                const uint8_t g0 = gray(ww.x, px), g1 = gray(ww.y, px + 1), g2 = gray(ww.z, px + 2), g3 = gray(ww.w, px + 3);
                const size_t yy = px / (size_t)so.W, xx = px - yy * (size_t)so.W;
                if (xx + 3 < (size_t)so.W && ((so.stride | (long long)xx) & 3) == 0 && (reinterpret_cast<uintptr_t>(so.out) & 3) == 0) {
                    *reinterpret_cast<unsigned*>(so.out + yy * so.stride + xx) =
                        (unsigned)g0 | ((unsigned)g1 << 8) | ((unsigned)g2 << 16) | ((unsigned)g3 << 24);
                } else {   // a group of 4 that straddles two rows, or an unaligned frame
                    const uint8_t gg[4] = {g0, g1, g2, g3};
                    for (int q = 0; q < 4; q++) {
                        const size_t pq = px + q, yq = pq / (size_t)so.W, xq = pq - yq * (size_t)so.W;
                        so.out[yq * so.stride + xq] = gg[q];
                    }
                }
            }
        } else {
            for (size_t j = 4 * i; j < n; j++) {
                const unsigned m = mask[j], mh = mask_hi ? mask_hi[j] : 0u;
                mask[j] = 0;
                if (mask_hi) mask_hi[j] = 0;
                const float wj = one(w[j], m, mh, j);
                w[j] = wj;
                if (so.out) so.out[(j / (size_t)so.W) * so.stride + j % (size_t)so.W] = gray(wj, j);
            }
        }
    }
}

// Temporal-prior surface as an 8-bit frame.
//   mode 0  the reference's bridge from device state to the gating input, g = uint8(clip(-3366 / log10(I) - 306, 0,
//           255)) with I = V_ds / R, V_ds = 1 V (optical_flow_seg.py:426-431, simulationcode_v4_transistor_uav.m:36),
//           evaluated per pixel in double on R = resistance_exp(w) as float32.  Calibrated for arrays that start at
//           w = 0: the event simulator's initial state w = 0.5 (I = 1.7 uA) already maps to 255.
//   mode 1  build-defined linear map of the state itself, g = uint8(255 * w) (float32 product, truncated): the frame
//           the joined events -> surface -> flow pipeline (BASELINE config 5) hands to the flow stage.
//   ResT  DevF (one device) or MapRes (per-pixel resistance constants)
template <class ResT>
__global__ __launch_bounds__(256) void k_surface_gray(const float* __restrict__ w, uint8_t* __restrict__ out, int W, int H,
                                                       ptrdiff_t stride, ResT p, int mode)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W || y >= H) return;
    const size_t pix = (size_t)y * W + x;
    out[(ptrdiff_t)y * stride + x] = surface_gray_one(w[pix], res_at(p, pix, mode), mode);
}

// The same surface as a float frame: g rounded to float32 instead of truncated to 8 bits (finite, in [0, 255]).
template <class ResT>
__global__ __launch_bounds__(256) void k_surface_gray_f32(const float* __restrict__ w, float* __restrict__ out, int W, int H,
                                                           ptrdiff_t stride, ResT p, int mode)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= W || y >= H) return;
    const size_t pix = (size_t)y * W + x;
    reinterpret_cast<float*>(reinterpret_cast<char*>(out) + (ptrdiff_t)y * stride)[x] =
        (float)surface_gray_value(w[pix], res_at(p, pix, mode), mode);
}

// ---- surface frames as copy + patch -------------------------------------------------------------------------------------
// With the silent voltage in the dead zone a pixel without events keeps its state bit for bit, so the 8-bit frame of interval
// k differs from that of interval k-1 only at the pixels the interval's events touch (0.4 % of a 3840x2160 sensor at 1 M
// events/s and 33 ms per frame).  The every-pixel pass moves 17 B/px per interval to find that out; here an interval is
//   A  k_frames_scatter_copy   frames[k] = frames[k-1] (2 B/px) while the interval's events are scattered into the per-pixel
//                              slice masks (one 64-bit word: up to 64 slices) and the compact list of touched pixels
//   B  k_update_list           the touched pixels replay their slices in order, store w and overwrite their byte of frames[k]
// -- same states, same frames (tests/test_accum_gpu.py::test_run_frames_copy_patch_equals_dense_frames).
//   COUNT  theta > 1: counter fields in the 64-bit word (intervals of up to 64 / th.bits slices)
template <bool COUNT>
__global__ __launch_bounds__(256) void k_frames_scatter_copy(const uint8_t* __restrict__ prev, uint8_t* __restrict__ cur, int W, int H,
                                                              long long row_stride, const short* __restrict__ x,
                                                              const short* __restrict__ y, long long ev0, long long n_ev,
                                                              const long long* __restrict__ bounds, int n_sl,
                                                              unsigned long long* mask64, unsigned* list, unsigned* count,
                                                              ThetaArg<COUNT> th)
{
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nthreads = (long long)gridDim.x * 256;
    // the events of the interval FIRST (their atomics' latency then overlaps the copy; whole waves take part: the list append
    // is aggregated per wave)
    const long long n_ev_pad = (n_ev + 63) & ~63ll;
    for (long long i = tid; i < n_ev_pad; i += nthreads) {
        const bool live = i < n_ev;
        const long long e = ev0 + (live ? i : 0);
        if constexpr (COUNT)
            mark_count(mask64, list, count, (unsigned)y[e] * (unsigned)W + (unsigned)x[e], slice_of(bounds, n_sl, e) * th.bits, th, live);
        else
            mark(mask64, list, count, (unsigned)y[e] * (unsigned)W + (unsigned)x[e], 1ull << slice_of(bounds, n_sl, e), live);
    }
    // ... then this thread's share of the copy
    if (prev) {
        if (row_stride == W && (((size_t)W * H) & 15) == 0 && ((reinterpret_cast<uintptr_t>(prev) | reinterpret_cast<uintptr_t>(cur)) & 15) == 0) {
            const long long n16 = (long long)W * H / 16;
            typedef unsigned u4v __attribute__((ext_vector_type(4)));
            const u4v* s4 = reinterpret_cast<const u4v*>(prev);
            u4v* d4 = reinterpret_cast<u4v*>(cur);
            for (long long i = tid; i < n16; i += nthreads) __builtin_nontemporal_store(s4[i], d4 + i);
        } else {
            const long long n = (long long)W * H;
            for (long long i = tid; i < n; i += nthreads) {
                const long long yy = i / W, xx = i - yy * W;
                cur[yy * row_stride + xx] = prev[yy * row_stride + xx];
            }
        }
    }
}

// ---- surface frames by a tile-persistent walk ---------------------------------------------------------------------
// Pixels never interact, so nothing forces an interval to be a launch: a WAVE owns a tile of 1024 consecutive pixels for
// the WHOLE run.  Its state (w, 4 KB), the 8-bit bytes of the current frame (1 KB) and a 64-bit slice mask per pixel (8 KB)
// live in LDS; per interval it ORs the tile's events into the masks, lets one lane per touched pixel replay them
// (atomicExch claims the mask), and streams the tile's 1 KB of frame k out -- frames are WRITE-ONLY (1 B/px per frame, no
// read of the previous frame), the state is read and written once per run:
//   k_tile_bucket   the run's events bucketed by (interval, tile): records of 16 bits (pixel in tile, slice in interval);
//                   the order inside a bucket is irrelevant (scheme 1 applies the same drive once per distinct active slice)
//   k_tile_frames   the walk
// -- two launches per call.
constexpr int TILE_PX = 1024, TILE_SHIFT = 10;

// One workgroup per interval buckets that interval's events by tile: the events of interval k are the contiguous range
// [bounds[k * every], bounds[(k + 1) * every]) of the time-sorted stream and their records fill exactly that range of recs,
// so the counting sort is local -- histogram over the tiles in LDS, exclusive scan, fill through LDS cursors -- and no
// global scan or global atomic is needed.  off[k * ntiles + t] = start of bucket (k, t) in recs; off[n_frames * ntiles] = n_ev.
__global__ __launch_bounds__(1024) void k_tile_bucket(const short* __restrict__ x, const short* __restrict__ y, long long ev0,
                                                       const long long* __restrict__ bounds, int every, int W, unsigned ntiles,
                                                       unsigned* __restrict__ off, unsigned short* __restrict__ recs, int n_frames)
{
    extern __shared__ unsigned s_cnt[];           // [ntiles]
    __shared__ long long s_b[65];                 // the interval's slice bounds (event indices)
    __shared__ unsigned s_part[1024];
    const int k = blockIdx.x, tid = threadIdx.x;
    for (unsigned t = tid; t < ntiles; t += 1024) s_cnt[t] = 0;
    if (tid <= every) s_b[tid] = bounds[(size_t)k * every + tid];
    __syncthreads();
    const long long lo = s_b[0], hi = s_b[every];
    const unsigned base = (unsigned)(lo - ev0);
    auto rec_of = [&](long long e, unsigned& tile) -> unsigned {
        const unsigned s = (unsigned)slice_of(s_b, every, e);
        const unsigned pix = (unsigned)y[e] * (unsigned)W + (unsigned)x[e];
        tile = pix >> TILE_SHIFT;
        return (pix & (TILE_PX - 1)) | (s << TILE_SHIFT);
    };
    for (long long e = lo + tid; e < hi; e += 1024) {
        unsigned tile;
        (void)rec_of(e, tile);
        atomicAdd(&s_cnt[tile], 1u);
    }
    __syncthreads();
    // exclusive scan over the tiles: thread i owns tiles [i * per, (i + 1) * per)
    const unsigned per = (ntiles + 1023) / 1024, t0 = tid * per, t1 = min(t0 + per, ntiles);
    unsigned sum = 0;
    for (unsigned t = t0; t < t1; t++) sum += s_cnt[t];
    s_part[tid] = sum;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1) {
        const unsigned v = tid >= (int)d ? s_part[tid - d] : 0;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    unsigned run = s_part[tid] - sum;
    for (unsigned t = t0; t < t1; t++) {
        const unsigned c = s_cnt[t];
        off[(size_t)k * ntiles + t] = base + run;
        s_cnt[t] = run;                           // the fill pass's cursor
        run += c;
    }
    if (k == n_frames - 1 && tid == 0) off[(size_t)n_frames * ntiles] = (unsigned)(hi - ev0);
    __syncthreads();
    for (long long e = lo + tid; e < hi; e += 1024) {
        unsigned tile;
        const unsigned rec = rec_of(e, tile);
        recs[base + atomicAdd(&s_cnt[tile], 1u)] = (unsigned short)rec;
    }
}

// (MK_FITTED / MK_UNIFORM only: a mapped accumulator takes copy + patch, see nsof_accum_run_frames)
template <int KIND>
__global__ __launch_bounds__(256) void k_tile_frames(float* __restrict__ w, size_t npx, int W, const unsigned* __restrict__ off,
                                                      const unsigned short* __restrict__ recs, unsigned ntiles, int n_frames,
                                                      float v_act, uint8_t* __restrict__ frames, long long row_stride,
                                                      long long frame_stride, ModelArg<KIND> model, int mode)
{
    const DevF p = model_arg(model);
    __shared__ unsigned long long s_mask[4][TILE_PX];
    __shared__ __attribute__((aligned(16))) float s_w[4][TILE_PX];
    __shared__ __attribute__((aligned(16))) uint8_t s_b[4][TILE_PX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const unsigned tile = blockIdx.x * 4 + wv;
    if (tile >= ntiles) return;                                   // wave-uniform; no block barrier below
    unsigned long long* ml = s_mask[wv];
    float* wl = s_w[wv];
    uint8_t* bl = s_b[wv];
    const size_t p0 = (size_t)tile * TILE_PX + (size_t)lane * 16;   // this lane's 16 pixels (one row: W % 16 == 0)
    const bool live = p0 < npx;
    const size_t yy = live ? p0 / (size_t)W : 0, xx = live ? p0 - yy * (size_t)W : 0;
    typedef float f4v __attribute__((ext_vector_type(4)));
    typedef unsigned u4v __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int j = 0; j < 4; j++) {
        f4v v = live ? reinterpret_cast<const f4v*>(w + p0)[j] : (f4v){0.f, 0.f, 0.f, 0.f};
        reinterpret_cast<f4v*>(wl + lane * 16)[j] = v;
#pragma unroll
        for (int q = 0; q < 4; q++) bl[lane * 16 + 4 * j + q] = surface_gray_one(v[q], p, mode);
    }
#pragma unroll
    for (int j = 0; j < 16; j++) ml[lane * 16 + j] = 0ull;
    const Drive da = drive_of(v_act, p);
    bool dirty = false;
    for (int kb = 0; kb < n_frames; kb += 63) {
        // the bucket bounds of up to 63 intervals of this tile, one per lane (lane i: the start of interval kb + i)
        // (buckets are laid out interval-major: bucket (k, tile) = recs[off[k * ntiles + tile] .. off[k * ntiles + tile + 1]))
        const int kn = min(63, n_frames - kb);
        const unsigned mybeg = lane < kn ? off[(size_t)(kb + lane) * ntiles + tile] : 0u;
        const unsigned myend = lane < kn ? off[(size_t)(kb + lane) * ntiles + tile + 1] : 0u;
        // the first 64 records of the next PF intervals are in flight (a record load is ~1 us of L2 latency against ~0.15 us
        // of work per interval)
        constexpr int PF = 4;
        unsigned rq[PF];
#pragma unroll
        for (int d = 0; d < PF; d++) {
            const unsigned qb = d < kn ? __builtin_amdgcn_readlane(mybeg, d) : 0u, qe = d < kn ? __builtin_amdgcn_readlane(myend, d) : 0u;
            rq[d] = qb + lane < qe ? recs[qb + lane] : 0xffffffffu;
        }
        for (int i0 = 0; i0 < kn; i0 += PF) {
#pragma unroll
          for (int d = 0; d < PF; d++) {
            const int i = i0 + d;
            if (i >= kn) break;                                   // wave-uniform
            const unsigned rcur = rq[d];
            const unsigned c0 = __builtin_amdgcn_readlane(mybeg, i), c1 = __builtin_amdgcn_readlane(myend, i);
            if (i + PF < kn) {
                const unsigned qb = __builtin_amdgcn_readlane(mybeg, i + PF), qe = __builtin_amdgcn_readlane(myend, i + PF);
                rq[d] = qb + lane < qe ? recs[qb + lane] : 0xffffffffu;
            }
            if (c1 > c0) {                                        // wave-uniform
                dirty = true;
                // pass 1: every event of the bucket marks (pixel, slice)
                if (rcur != 0xffffffffu) atomicOr(&ml[rcur & (TILE_PX - 1)], 1ull << (rcur >> TILE_SHIFT));
                for (unsigned q = c0 + 64 + lane; q < c1; q += 64) {
                    const unsigned r = recs[q];
                    atomicOr(&ml[r & (TILE_PX - 1)], 1ull << (r >> TILE_SHIFT));
                }
                // pass 2: one lane per touched pixel claims its mask and replays the slices (LDS operations of a wave
                // execute in order: every mark above is visible here; the fences keep the compiler from moving them)
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                auto settle = [&](unsigned r) {
                    const unsigned pix = r & (TILE_PX - 1);
                    const unsigned long long m = atomicExch(&ml[pix], 0ull);
                    if (m) {
                        const float ww = replay_driven(wl[pix], m, da);
                        wl[pix] = ww;
                        bl[pix] = surface_gray_one(ww, p, mode);
                    }
                };
                if (rcur != 0xffffffffu) settle(rcur);
                for (unsigned q = c0 + 64 + lane; q < c1; q += 64) settle(recs[q]);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
            if (live) {
                const u4v bytes = reinterpret_cast<const u4v*>(bl)[lane];
                __builtin_nontemporal_store(bytes, reinterpret_cast<u4v*>(frames + (size_t)(kb + i) * frame_stride + yy * row_stride + xx));
            }
          }
        }
    }
    if (dirty && live) {
#pragma unroll
        for (int j = 0; j < 4; j++) reinterpret_cast<f4v*>(w + p0)[j] = reinterpret_cast<const f4v*>(wl + lane * 16)[j];
    }
}

// bincount_2d (event_mem_sim.py:100-104): events per pixel.
__global__ __launch_bounds__(256) void k_bincount(const short* __restrict__ x, const short* __restrict__ y, size_t n,
                                                   int W, int* __restrict__ counts)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        atomicAdd(&counts[(size_t)y[i] * W + x[i]], 1);
}

// f(KindTag<MK_FITTED>, NoModel) for the fitted device, f(KindTag<MK_UNIFORM>, DevF) for another one, f(KindTag<MK_MAPPED>,
// MapF) with parameter maps: the kernel instantiation and its argument
template <class Fn>
void with_model(const Model& m, Fn&& f)
{
    if (m.mapped) f(KindTag<MK_MAPPED>{}, m.map);
    else if (m.fitted) f(KindTag<MK_FITTED>{}, NoModel{});
    else f(KindTag<MK_UNIFORM>{}, m.f);
}
// ... for the kernels that have no mapped form (the tile walk): the caller has routed a mapped accumulator elsewhere
template <class Fn>
void with_uniform_model(const Model& m, Fn&& f)
{
    if (m.fitted) f(KindTag<MK_FITTED>{}, NoModel{});
    else f(KindTag<MK_UNIFORM>{}, m.f);
}
// f(DevF) or f(MapRes): the argument of the kernels that read a pixel's resistance only
template <class Fn>
void with_res(const Model& m, Fn&& f)
{
    if (m.mapped) f(MapRes{m.map.res});
    else f(m.f);
}
}  // namespace

struct nsof_accum {
    nsof_ctx* ctx = nullptr;
    int H = 0, W = 0, scheme = 1, split = 0;
    float active_v = 0, silent_v = 0;
    int force_dense = 0;   // nsof_accum_set_dense: 0 automatic, 1 every-pixel pass, -1 event-pixel update (where exact)
    int theta = 1;         // nsof_accum_set_event_threshold: scheme 1's THETA_EVENTS
    size_t npx = 0;
    nsof_dev_buf<float> w[2];
    nsof_dev_buf<long long> next_ok[2];
    nsof_dev_buf<unsigned> mask[2];
    nsof_dev_buf<unsigned> mask_hi;   // slices 32..63 of a dense scheme-1 group (allocated on first use, kept zero between groups)
    nsof_dev_buf<unsigned long long> mask64;   // nsof_accum_run_frames (copy + patch): one 64-bit slice mask per pixel
    // nsof_accum_run_frames (tile walk): bucket offsets [intervals * tiles + 1] and the 16-bit event records
    nsof_dev_buf<unsigned> tile_off;
    nsof_dev_buf<unsigned short> tile_recs;
    nsof_dev_buf<unsigned> list[2];
    nsof_dev_buf<unsigned> count;  // [2]
    StagedStream ev;   // nsof_accum_set_events / the staging half of nsof_accum_step_events
    // snapshots
    nsof_dev_buf<float> snap[2];
    int64_t snap_cap = 0, snap_count = 0;
    int64_t slice_counter = 0;
    Model model;             // the device the array is made of (nsof_accum_create_p): the scalars are fixed for the accumulator's life
    // per-pixel parameter maps (nsof_accum_set_param_maps): the raw float32 planes of the mapped keys (kept for
    // nsof_accum_read_param_map; the wini plane is what reset copies) and what k_setup_maps made of them (model.map points here)
    unsigned map_mask = 0;
    bool map_dead_zone = false;   // silent_v inside [voff, von] at EVERY pixel
    nsof_dev_buf<float> map_plane[NSOF_ACCUM_KEY_COUNT];
    nsof_dev_buf<float> map_act, map_sil, map_res;
    int frames_path = 0;     // nsof_accum_run_frames: 0 = the tile walk where it applies, 1 = copy + patch per interval (kept as the cross-check)
};

extern "C" void nsof_accum_destroy(nsof_accum* a)
{
    if (!a) return;
    hipSetDevice(a->ctx->device);
    hipStreamSynchronize(a->ctx->stream);
    delete a;
}

extern "C" int nsof_accum_reset(nsof_accum* a)
{
    if (!a) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const int narr = a->split ? 2 : 1;
    for (int i = 0; i < narr; i++) {
        if (a->map_mask >> NSOF_ACCUM_KEY_WINI & 1u)
            NSOF_HIP(ctx, hipMemcpyAsync(a->w[i].p, a->map_plane[NSOF_ACCUM_KEY_WINI].p, a->npx * sizeof(float), hipMemcpyDeviceToDevice,
                                         ctx->stream));
        else
            hipLaunchKernelGGL(k_fill, dim3(grid_for(a->npx)), dim3(256), 0, ctx->stream, a->w[i].p, a->npx, a->model.wini_f);
        NSOF_HIP(ctx, hipMemsetAsync(a->mask[i].p, 0, a->npx * sizeof(unsigned), ctx->stream));
        if (a->scheme == 2) NSOF_HIP(ctx, hipMemsetAsync(a->next_ok[i].p, 0, a->npx * sizeof(long long), ctx->stream));
    }
    NSOF_HIP(ctx, hipGetLastError());
    a->slice_counter = 0;
    a->snap_count = 0;
    return NSOF_OK;
}

// Per-pixel parameter maps: see include/nsof.h.  Everything that can refuse the call -- the accumulator's state, the plane list,
// the domain of every pixel of every plane (plane_set_of, with one trial) -- is decided on the host before the accumulator or
// the device is touched; the new planes are allocated aside and swapped in only once they are all there.
extern "C" int nsof_accum_set_param_maps(nsof_accum* a, int n_maps, const int* keys, const float* const* maps)
{
    if (!a) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (a->slice_counter != 0 || a->snap_count != 0)
        return nsof_set_error(ctx, NSOF_EINVAL, "set_param_maps: the accumulator has advanced (slice %lld, %lld snapshots); reset it first",
                              (long long)a->slice_counter, (long long)a->snap_count);
    const Model& mo = a->model;
    const size_t npx = a->npx;
    int one_trial[NSOF_ACCUM_KEY_COUNT];
    std::fill(one_trial, one_trial + NSOF_ACCUM_KEY_COUNT, 1);
    PlaneSet<float> ps;
    if (int rc = plane_set_of(ctx, PlaneLabels{"set_param_maps", "parameter map"}, mo, a->H, a->W, 1, n_maps, keys, maps, one_trial, &ps))
        return rc;
    // what decides between the event-pixel update / the no-op silent slices and the every-pixel pass with a per-pixel
    // silent drive
    const bool dead = silent_in_every_dead_zone(ps, mo.f, a->silent_v, npx);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    if (n_maps == 0) {   // back to the uniform model (the planes stay allocated for a later call)
        a->map_mask = 0;
        a->model.mapped = false;
        a->model.map = MapF{nullptr, nullptr, nullptr, 0.f};
        return nsof_accum_reset(a);
    }
    nsof_dev_buf<float> np_[NSOF_ACCUM_KEY_COUNT], nact, nsil, nres;
    int rc = nact.reserve(ctx, npx * 3 * sizeof(float));
    if (!rc) rc = nsil.reserve(ctx, npx * 3 * sizeof(float));
    if (!rc) rc = nres.reserve(ctx, npx * 2 * sizeof(float));
    MapSrc src;
    if (!rc) rc = upload_planes(ctx, mo, ps, npx, np_, &src);
    if (rc) return rc;
    unsigned mask = 0;
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++)
        if (ps.plane[k]) mask |= 1u << k;
    const float v_act = a->scheme == 1 ? a->active_v : a->silent_v + a->active_v;
    // (one trial; the state is nsof_accum_reset's, below)
    hipLaunchKernelGGL(k_setup_maps, dim3(grid_for(npx)), dim3(256), 0, ctx->stream, src, npx, 1, v_act, a->silent_v, nact.p, nsil.p,
                       reinterpret_cast<float2*>(nres.p), (float*)nullptr, (float*)nullptr, (const float*)nullptr, (const float*)nullptr);
    NSOF_HIP(ctx, hipGetLastError());
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));   // the caller's planes are not retained; the old ones are free to go
    for (int k = 0; k < NSOF_ACCUM_KEY_COUNT; k++) a->map_plane[k].swap(np_[k]);
    a->map_act.swap(nact);
    a->map_sil.swap(nsil);
    a->map_res.swap(nres);
    a->map_mask = mask;
    a->map_dead_zone = dead;
    a->model.mapped = true;
    a->model.map = MapF{a->map_act.p, a->map_sil.p, reinterpret_cast<const float2*>(a->map_res.p), mo.f.dt};
    return nsof_accum_reset(a);
}

extern "C" int nsof_accum_read_param_map(nsof_accum* a, int key, float* out)
{
    if (!a || !out) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (key < 0 || key >= NSOF_ACCUM_KEY_COUNT || !(a->map_mask >> key & 1u))
        return nsof_set_error(ctx, NSOF_EINVAL, "read_param_map: key %d is uniform (no map set)", key);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    NSOF_HIP(ctx, hipMemcpyAsync(out, a->map_plane[key].p, a->npx * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NSOF_OK;
}

extern "C" int nsof_accum_param_map_mask(const nsof_accum* a, unsigned* mask)
{
    if (!a || !mask) return NSOF_EINVAL;
    *mask = a->map_mask;
    return NSOF_OK;
}

extern "C" void nsof_accum_default_params(nsof_accum_params* out)
{
    if (out) *out = default_params();
}

extern "C" int nsof_accum_get_params(const nsof_accum* a, nsof_accum_params* out)
{
    if (!a || !out) return NSOF_EINVAL;
    *out = a->model.prm;
    return NSOF_OK;
}

extern "C" int nsof_accum_create(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v,
                                 float silent_v, nsof_accum** out)
{
    return nsof_accum_create_p(ctx, height, width, scheme, polarity_split, active_v, silent_v, nullptr, out);
}

extern "C" int nsof_accum_create_p(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v,
                                   float silent_v, const nsof_accum_params* params, nsof_accum** out)
{
    if (!ctx || !out) return NSOF_EINVAL;
    *out = nullptr;
    Model model;
    if (int rc = model_of(ctx, params, &model)) return rc;
    if (height < 1 || width < 1 || (scheme != 1 && scheme != 2))
        return nsof_set_error(ctx, NSOF_EINVAL, "bad accumulator geometry %dx%d or scheme %d", height, width, scheme);
    if ((size_t)height * width > 0xFFFFFFFFull) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "sensor too large");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    nsof_accum* a = new (std::nothrow) nsof_accum();
    if (!a) return nsof_set_error(ctx, NSOF_ENOMEM, "out of host memory");
    a->ctx = ctx; a->H = height; a->W = width; a->scheme = scheme;
    a->model = model;
    a->split = (scheme == 2 && polarity_split) ? 1 : 0;
    a->active_v = active_v; a->silent_v = silent_v;
    a->npx = (size_t)height * width;
    const int narr = a->split ? 2 : 1;
    int rc = a->count.reserve(ctx, 4 * sizeof(unsigned));   // [parity][array]: groups alternate, see accum_advance
    for (int i = 0; i < narr && !rc; i++) {
        rc = a->w[i].reserve(ctx, (a->npx + 4) * sizeof(float));
        if (!rc) rc = a->mask[i].reserve(ctx, (a->npx + 4) * sizeof(unsigned));
        if (!rc && scheme == 2) rc = a->next_ok[i].reserve(ctx, a->npx * sizeof(long long));
    }
    if (!rc) rc = nsof_accum_reset(a);
    if (rc) { nsof_accum_destroy(a); return rc; }
    *out = a;
    return NSOF_OK;
}

extern "C" int nsof_accum_set_frames_path(nsof_accum* a, int path)
{
    if (!a || path < 0 || path > 1) return NSOF_EINVAL;
    a->frames_path = path;
    return NSOF_OK;
}

extern "C" int nsof_accum_set_dense(nsof_accum* a, int force_dense)
{
    if (!a) return NSOF_EINVAL;
    a->force_dense = force_dense > 0 ? 1 : (force_dense < 0 ? -1 : 0);
    return NSOF_OK;
}

extern "C" int nsof_accum_set_event_threshold(nsof_accum* a, int theta)
{
    if (!a) return NSOF_EINVAL;
    if (theta < 1) return nsof_set_error(a->ctx, NSOF_EINVAL, "event threshold %d: at least 1 event", theta);
    if (a->scheme == 2 && theta != 1)
        return nsof_set_error(a->ctx, NSOF_EINVAL, "event threshold %d: scheme 2 has no count threshold (only 1 is accepted)", theta);
    a->theta = theta;
    return NSOF_OK;
}

extern "C" int nsof_accum_get_event_threshold(const nsof_accum* a, int* theta)
{
    if (!a || !theta) return NSOF_EINVAL;
    *theta = a->theta;
    return NSOF_OK;
}

static int accum_snapshot(nsof_accum* a)
{
    nsof_ctx* ctx = a->ctx;
    const int narr = a->split ? 2 : 1;
    if (a->snap_count == a->snap_cap) {
        const int64_t ncap = a->snap_cap ? a->snap_cap * 2 : 16;
        for (int i = 0; i < narr; i++) {
            nsof_dev_buf<float> nb;
            if (int rc = nb.reserve(ctx, (size_t)ncap * a->npx * sizeof(float))) return rc;
            if (a->snap_count)
                NSOF_HIP(ctx, hipMemcpyAsync(nb.p, a->snap[i].p, (size_t)a->snap_count * a->npx * sizeof(float),
                                             hipMemcpyDeviceToDevice, ctx->stream));
            NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
            a->snap[i].swap(nb);   // the old array goes with nb
        }
        a->snap_cap = ncap;
    }
    for (int i = 0; i < narr; i++)
        with_res(a->model, [&](auto res) {
            hipLaunchKernelGGL(k_resistance<decltype(res)>, dim3(grid_for(a->npx)), dim3(256), 0, ctx->stream, a->w[i].p,
                               a->snap[i].p + (size_t)a->snap_count * a->npx, a->npx, res);
        });
    NSOF_HIP(ctx, hipGetLastError());
    a->snap_count++;
    return NSOF_OK;
}

// Stage the events of slices [0, n_slices) (StagedStream) and make room for the lists of touched pixels.
// n_dev >= 0: the arrays are DEVICE memory holding n_dev events (StagedStream::stage_dev).
static int accum_stage(nsof_accum* a, const int16_t* x, const int16_t* y, const int8_t* p, const int64_t* t,
                       const int64_t* sb, int64_t n_slices, int64_t n_dev = -1)
{
    nsof_ctx* ctx = a->ctx;
    const long long refr = a->model.prm.refractory_us;
    if (int rc = n_dev >= 0 ? a->ev.stage_dev(ctx, a->W, a->H, a->scheme, a->split, refr, x, y, p, t, n_dev, sb, n_slices)
                            : a->ev.stage(ctx, a->W, a->H, a->scheme, a->split, refr, x, y, p, t, sb, n_slices))
        return rc;
    const size_t n_ev = (size_t)a->ev.rel.back();
    int rc = NSOF_OK;
    for (int i = 0; i < (a->split ? 2 : 1) && !rc; i++)
        rc = a->list[i].reserve(ctx, n_ev * sizeof(unsigned), StagedStream::event_cap((int64_t)n_ev) * sizeof(unsigned));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the caller's arrays are not retained
    return rc;
}

// Scheme 2 reads two timestamps per slice -- its first event's (the refractory test, event_mem_sim.py:243,253,265) and
// its last event's (+ refractory_us -> next_ok, :246,256,267) -- and they belong to the slice of the WHOLE stream.  A
// row band (nsof.dist.simulate_banded) stages only its own events, whose first / last differ: the caller hands the
// global table over, and the band's state then equals its rows of the unsharded run.
extern "C" int nsof_accum_set_slice_times(nsof_accum* a, const int64_t* t_first, const int64_t* t_last, int64_t n_slices)
{
    if (!a) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (!t_first || !t_last || n_slices != (int64_t)a->ev.tfirst.size())
        return nsof_set_error(ctx, NSOF_EINVAL, "set_slice_times: %lld slices given, %zu staged", (long long)n_slices, a->ev.tfirst.size());
    if (a->scheme != 2) return NSOF_OK;   // scheme 1 reads no timestamps
    for (int64_t s = 0; s < n_slices; s++) {
        a->ev.tfirst[s] = t_first[s];
        a->ev.tnext[s] = t_last[s] + a->model.prm.refractory_us;
    }
    return NSOF_OK;
}

// The silent voltage leaves an idle pixel bit for bit unchanged: the float32 comparisons update_one makes.
static bool dead_zone_of(const nsof_accum* a)
{
    if (a->model.mapped) return a->map_dead_zone;   // ... at every pixel (nsof_accum_set_param_maps)
    return !(a->silent_v < a->model.f.voff) && !(a->silent_v > a->model.f.von);
}

// The arguments every 8-bit surface entry point takes: an array of this accumulator, a surface mode, rows of at least W bytes.
static bool surface_args_ok(const nsof_accum* a, int which, int mode, const uint8_t* d_out, ptrdiff_t row_stride)
{
    return a && d_out && which >= 0 && which <= (a->split ? 1 : 0) && row_stride >= a->W && mode >= 0 && mode <= 1;
}

static int accum_surface(nsof_accum* a, int which, const SurfOut& so)
{
    nsof_ctx* ctx = a->ctx;
    dim3 grid((a->W + 255) / 256, a->H);
    with_res(a->model, [&](auto res) {
        hipLaunchKernelGGL(k_surface_gray<decltype(res)>, grid, dim3(256), 0, ctx->stream, a->w[which].p, so.out, a->W, a->H,
                           (ptrdiff_t)so.stride, res, so.mode);
    });
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// Advance over staged slices [s_begin, s_begin + n_slices).
// surf (optional): after the LAST slice of the call the surface of array surf_which goes to surf->out as an 8-bit frame --
// fused into the last group's dense scheme-1 update where that kernel runs, a separate k_surface_gray launch otherwise.
static int accum_advance(nsof_accum* a, int64_t s_begin, int64_t n_slices, int64_t snap_every, const SurfOut* surf = nullptr,
                         int surf_which = 0)
{
    nsof_ctx* ctx = a->ctx;
    if (s_begin < 0 || n_slices < 0 || (size_t)(s_begin + n_slices + 1) > a->ev.rel.size())
        return nsof_set_error(ctx, NSOF_EINVAL, "slices [%lld, %lld) outside the staged stream", (long long)s_begin,
                              (long long)(s_begin + n_slices));
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const int narr = a->split ? 2 : 1;
    int rc;
    const std::vector<long long>& rel = a->ev.rel;
    const bool dead_zone = dead_zone_of(a);
    // Scheme 1 with the silent voltage in the dead zone: the event-pixel update (lists, groups of 32 slices) and the
    // every-pixel pass (groups of 64 slices, no lists) give the same bits; which one is faster depends on the sensor size.
    // Measured with a frame every 33 slices (scripts/accum_mode_probe.py): 1280x720 0.39 vs 0.75-0.89 ms per 30 frames,
    // 3840x2160 0.97 vs 1.21 ms for the every-pixel pass -- both are launch bound and it needs half the launches; its cost
    // grows with the pixel count (16 B/px per 64 slices), so beyond ~12 M pixels the event-pixel update takes over.
    const size_t auto_dense_px = (size_t)12 << 20;
    const bool sparse = dead_zone && a->force_dense <= 0 && (a->force_dense < 0 || !(a->scheme == 1 && a->npx <= auto_dense_px));
    const float v_act = a->scheme == 1 ? a->active_v : a->silent_v + a->active_v;

    int64_t s0 = s_begin;
    const int64_t s_end = s_begin + n_slices;
    bool surf_done = false;
    // the dense scheme-1 update takes groups of up to 64 slices (two mask words per pixel): a 33-slice frame interval is one
    // pass over the array instead of two
    const bool wide = a->scheme == 1 && !sparse;
    if (wide && !a->mask_hi.p) {
        if ((rc = a->mask_hi.reserve(ctx, a->npx * sizeof(unsigned) + 16))) return rc;
        NSOF_HIP(ctx, hipMemsetAsync(a->mask_hi.p, 0, a->npx * sizeof(unsigned) + 16, ctx->stream));
    }
    // theta > 1: a mask word carries 32 / bits slices (Theta), so the groups are that much shorter
    const int64_t word_slices = a->theta == 1 ? MAX_GROUP : theta_of(a->theta).spw;
    const int64_t max_group = wide ? 2 * word_slices : word_slices;
    ListCounts cnt{a->count.p};
    if (sparse && s0 < s_end) NSOF_HIP(ctx, cnt.zero_all(ctx->stream));
    while (s0 < s_end) {
        const int64_t g = group_len(s0, s_end, max_group, snap_every, a->slice_counter);
        const long long ge0 = rel[s0], ge1 = rel[s0 + g], gn = ge1 - ge0;
        if (sparse && gn == 0) NSOF_HIP(ctx, hipMemsetAsync(cnt.next(), 0, 2 * sizeof(unsigned), ctx->stream));   // no update kernel will
        if (gn > 0) {
            nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
            unsigned* const l0 = sparse ? a->list[0].p : nullptr;   // the every-pixel update reads no list
            unsigned* const l1 = sparse ? a->list[a->split].p : nullptr;
            with_theta(a->theta, [&](auto C, auto th) {
                hipLaunchKernelGGL(k_scatter<decltype(C)::value>, dim3((unsigned)((gn + 255) / 256)), dim3(256), 0, ctx->stream, a->ev.dx.p,
                                   a->ev.dy.p, a->ev.dp.p, ge0, gn, a->ev.dbounds.p + s0, (int)g, a->W, a->split, a->mask[0].p, l0, cnt.cur(),
                                   a->mask[a->split].p, l1, cnt.cur() + 1, a->mask_hi.p, th);
            });
            NSOF_HIP(ctx, hipGetLastError());
        }
        {
            nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
            // array i of the group; R: std::true_type for scheme 2, whose kernels take the group's refractory table
            // C: std::true_type for a count threshold (scheme 1 only: the setter refuses it for scheme 2)
            auto update_c = [&](auto R, const auto& tab, int i, auto C, auto th) {
                constexpr bool REFR = decltype(R)::value, COUNT = decltype(C)::value;
                if constexpr (REFR && COUNT) return;
                else {
                SurfOut so{nullptr, 0, a->W, 0};
                if (sparse) {
                    if (gn > 0)
                        with_model(a->model, [&](auto D, auto model) {
                            hipLaunchKernelGGL((k_update_list<REFR, unsigned, false, decltype(D)::value, COUNT>),
                                               dim3(grid_for((size_t)gn, 1024)), dim3(256), 0, ctx->stream, a->w[i].p, a->mask[i].p,
                                               a->next_ok[i].p, a->list[i].p, cnt.cur() + i, tab, v_act, cnt.next() + i, so, model, th);
                        });
                    return;
                }
                if (wide && surf && i == surf_which && s0 + g == s_end) {   // the call's last group: leave the frame as well
                    so = *surf;
                    surf_done = true;
                }
                const size_t n4 = (a->npx + 3) / 4;
                with_model(a->model, [&](auto D, auto model) {
                    constexpr int KIND = decltype(D)::value;
                    auto* const kernel = dead_zone ? k_update_all<REFR, true, KIND, COUNT> : k_update_all<REFR, false, KIND, COUNT>;
                    hipLaunchKernelGGL(kernel, dim3(grid_for(n4, 8192)), dim3(256), 0, ctx->stream, a->w[i].p, a->mask[i].p,
                                       g > word_slices ? a->mask_hi.p : nullptr, a->next_ok[i].p, n4, a->npx, (int)g, tab, v_act,
                                       a->silent_v, so, model, th);
                });
                }
            };
            auto update = [&](auto R, const auto& tab, int i) {
                with_theta(a->theta, [&](auto C, auto th) { update_c(R, tab, i, C, th); });
            };
            if (a->scheme == 2) {
                const RefrTab tab = refr_tab_of(a->ev, s0, g);
                for (int i = 0; i < narr; i++) update(std::true_type{}, tab, i);
            } else {
                update(std::false_type{}, NoTab{}, 0);
            }
            NSOF_HIP(ctx, hipGetLastError());
        }
        a->slice_counter += g;
        s0 += g;
        if (sparse) cnt.flip();
        if (snapshot_due(a->slice_counter, snap_every))
            if ((rc = accum_snapshot(a))) return rc;
    }
    return surf && !surf_done ? accum_surface(a, surf_which, *surf) : NSOF_OK;
}

extern "C" int nsof_accum_step_events(nsof_accum* a, const int16_t* x, const int16_t* y, const int8_t* p,
                                      const int64_t* t, const int64_t* sb, int64_t n_slices, int64_t snap_every)
{
    if (!a) return NSOF_EINVAL;
    if (n_slices == 0) return NSOF_OK;
    if (int rc = accum_stage(a, x, y, p, t, sb, n_slices)) return rc;
    return accum_advance(a, 0, n_slices, snap_every);
}

extern "C" int nsof_accum_set_events(nsof_accum* a, const int16_t* x, const int16_t* y, const int8_t* p,
                                     const int64_t* t, const int64_t* sb, int64_t n_slices)
{
    if (!a) return NSOF_EINVAL;
    return accum_stage(a, x, y, p, t, sb, n_slices);
}

extern "C" int nsof_accum_step_events_dev(nsof_accum* a, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                                          int64_t n_events, const int64_t* sb, int64_t n_slices, int64_t snap_every)
{
    if (!a) return NSOF_EINVAL;
    if (n_events < 0) return nsof_set_error(a->ctx, NSOF_EINVAL, "a device stream of %lld events", (long long)n_events);
    if (n_slices == 0) return NSOF_OK;
    if (int rc = accum_stage(a, d_x, d_y, d_p, d_t, sb, n_slices, n_events)) return rc;
    return accum_advance(a, 0, n_slices, snap_every);
}

extern "C" int nsof_accum_set_events_dev(nsof_accum* a, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                                         int64_t n_events, const int64_t* sb, int64_t n_slices)
{
    if (!a) return NSOF_EINVAL;
    if (n_events < 0) return nsof_set_error(a->ctx, NSOF_EINVAL, "a device stream of %lld events", (long long)n_events);
    return accum_stage(a, d_x, d_y, d_p, d_t, sb, n_slices, n_events);
}

extern "C" int nsof_accum_run(nsof_accum* a, int64_t first_slice, int64_t n_slices, int64_t snap_every)
{
    if (!a) return NSOF_EINVAL;
    return accum_advance(a, first_slice, n_slices, snap_every);
}

extern "C" int nsof_accum_surface_u8_dev(nsof_accum* a, int which, int mode, uint8_t* d_out, ptrdiff_t row_stride)
{
    if (!surface_args_ok(a, which, mode, d_out, row_stride)) return NSOF_EINVAL;
    NSOF_HIP(a->ctx, hipSetDevice(a->ctx->device));
    return accum_surface(a, which, SurfOut{d_out, (long long)row_stride, a->W, mode});
}

extern "C" int nsof_accum_surface_f32_dev(nsof_accum* a, int which, int mode, float* d_out, ptrdiff_t row_stride_bytes)
{
    if (!a || !d_out || which < 0 || which > (a->split ? 1 : 0) || mode < 0 || mode > 1) return NSOF_EINVAL;
    if (row_stride_bytes < (ptrdiff_t)a->W * 4 || (row_stride_bytes & 3) || (reinterpret_cast<uintptr_t>(d_out) & 3))
        return nsof_set_error(a->ctx, NSOF_EINVAL, "surface_f32: row stride must be a multiple of 4 and >= 4*W, pointer 4-byte aligned");
    nsof_ctx* ctx = a->ctx;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    dim3 grid((a->W + 255) / 256, a->H);
    with_res(a->model, [&](auto res) {
        hipLaunchKernelGGL(k_surface_gray_f32<decltype(res)>, grid, dim3(256), 0, ctx->stream, a->w[which].p, d_out, a->W, a->H,
                           row_stride_bytes, res, mode);
    });
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_accum_run_surface(nsof_accum* a, int64_t first_slice, int64_t n_slices, int which, int mode, uint8_t* d_out,
                                      ptrdiff_t row_stride)
{
    if (!surface_args_ok(a, which, mode, d_out, row_stride)) return NSOF_EINVAL;
    const SurfOut so{d_out, (long long)row_stride, a->W, mode};
    return accum_advance(a, first_slice, n_slices, 0, &so, which);
}

// n_frames consecutive intervals of `every` slices, the surface after each into d_frames[k] (k-th frame at + k * frame_stride
// bytes).  Scheme 1 with the silent voltage in the dead zone and no forced every-pixel pass: frames as copy + patch (above),
// two small launches per interval issued from this one call; otherwise n_frames x nsof_accum_run_surface.
extern "C" int nsof_accum_run_frames(nsof_accum* a, int64_t first_slice, int64_t n_frames, int64_t every, int which, int mode,
                                     uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride)
{
    if (!surface_args_ok(a, which, mode, d_frames, row_stride) || n_frames < 0 || every < 1 || frame_stride < 0) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (n_frames == 0) return NSOF_OK;
    if (first_slice < 0 || (size_t)(first_slice + n_frames * every + 1) > a->ev.rel.size())
        return nsof_set_error(ctx, NSOF_EINVAL, "slices [%lld, %lld) outside the staged stream", (long long)first_slice,
                              (long long)(first_slice + n_frames * every));
    const bool dead_zone = dead_zone_of(a);
    // frame k of the call, as the kernels take it
    auto frame = [&](int64_t k) { return SurfOut{d_frames + k * frame_stride, (long long)row_stride, a->W, mode}; };
    // copy + patch scatters into ONE 64-bit word per pixel: 64 slices, or 64 / bits with a count threshold -- an interval
    // then takes ceil(every / word64_slices) rounds of (scatter, list update), the first of which copies the frame
    const int64_t word64_slices = a->theta == 1 ? 2 * MAX_GROUP : 64 / theta_of(a->theta).bits;
    if (!(a->scheme == 1 && dead_zone && a->force_dense <= 0 && every <= 2 * MAX_GROUP)) {
        for (int64_t k = 0; k < n_frames; k++) {
            const SurfOut so = frame(k);
            if (int rc = accum_advance(a, first_slice + k * every, every, 0, &so, which)) return rc;
        }
        return NSOF_OK;
    }
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    const std::vector<long long>& rel = a->ev.rel;
    const long long ev0 = rel[first_slice], n_ev = rel[first_slice + n_frames * every] - ev0;
    // ---- the tile walk: whole run in four launches (frames write-only); needs 16-byte-addressable frame rows
    const bool tile_ok = (a->W & 15) == 0 && (row_stride & 15) == 0 && (frame_stride & 15) == 0 &&
                         (reinterpret_cast<uintptr_t>(d_frames) & 15) == 0 && n_frames >= 2 && n_ev < (1ll << 31) &&
                         (a->npx + TILE_PX - 1) / TILE_PX <= 15000 &&   // the bucketing workgroup's histogram: 4 B per tile of LDS
                         (size_t)n_frames * ((a->npx + TILE_PX - 1) / TILE_PX) < ((size_t)1 << 30) && a->frames_path != 1 &&
                         a->theta == 1 &&   // the walk's LDS masks hold bits, not counts
                         !a->model.mapped;   // ... and its waves one drive: a mapped accumulator takes copy + patch
    if (tile_ok) {
        const unsigned ntiles = (unsigned)((a->npx + TILE_PX - 1) / TILE_PX);
        const size_t nb = (size_t)n_frames * ntiles;
        if ((rc = a->tile_off.reserve(ctx, (nb + 1) * 4, (nb + nb / 4 + 1024) * 4)) ||
            (rc = a->tile_recs.reserve(ctx, (size_t)n_ev * 2, ((size_t)n_ev + (size_t)n_ev / 4 + 1024) * 2)))
            return rc;
        nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
        hipLaunchKernelGGL(k_tile_bucket, dim3((unsigned)n_frames), dim3(1024), (size_t)ntiles * 4, ctx->stream, a->ev.dx.p, a->ev.dy.p, ev0,
                           a->ev.dbounds.p + first_slice, (int)every, a->W, ntiles, a->tile_off.p, a->tile_recs.p, (int)n_frames);
        with_uniform_model(a->model, [&](auto D, auto model) {
            hipLaunchKernelGGL(k_tile_frames<decltype(D)::value>, dim3((ntiles + 3) / 4), dim3(256), 0, ctx->stream, a->w[0].p, a->npx,
                               a->W, (const unsigned*)a->tile_off.p, (const unsigned short*)a->tile_recs.p, ntiles, (int)n_frames,
                               a->active_v, d_frames, (long long)row_stride, (long long)frame_stride, model, mode);
        });
        NSOF_HIP(ctx, hipGetLastError());
        a->slice_counter += n_frames * every;
        return NSOF_OK;
    }
    if (!a->mask64.p) {   // per-pixel 64-bit slice masks of this path (kept zero between intervals)
        if ((rc = a->mask64.reserve(ctx, a->npx * sizeof(unsigned long long)))) return rc;
        NSOF_HIP(ctx, hipMemsetAsync(a->mask64.p, 0, a->npx * sizeof(unsigned long long), ctx->stream));
    }
    ListCounts cnt{a->count.p};
    NSOF_HIP(ctx, cnt.zero_all(ctx->stream));
    constexpr size_t ACC_COPY_BLOCKS = 4096;
    const unsigned copy_blocks = (unsigned)std::min<size_t>(ACC_COPY_BLOCKS, (a->npx / 16 + 255) / 256 + 1);
    for (int64_t k = 0; k < n_frames; k++) {
        const SurfOut cur = frame(k);
        nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
        // theta == 1: one round, the whole interval.  A later round without events is skipped whole: the counter it would
        // append to is already zero and stays the current one.
        for (int64_t r0 = 0; r0 < every; r0 += word64_slices) {
            const int64_t s0 = first_slice + k * every + r0, rn = std::min<int64_t>(word64_slices, every - r0);
            const long long ge0 = rel[s0], gn = rel[s0 + rn] - ge0;
            if (r0 > 0 && gn == 0) continue;
            const uint8_t* const prev = k > 0 && r0 == 0 ? frame(k - 1).out : nullptr;
            if (prev || gn > 0) {
                const unsigned blocks = prev ? copy_blocks : (unsigned)((gn + 255) / 256);
                with_theta(a->theta, [&](auto C, auto th) {
                    hipLaunchKernelGGL(k_frames_scatter_copy<decltype(C)::value>, dim3(blocks), dim3(256), 0, ctx->stream, prev, cur.out,
                                       a->W, a->H, (long long)row_stride, a->ev.dx.p, a->ev.dy.p, ge0, gn, a->ev.dbounds.p + s0, (int)rn,
                                       a->mask64.p, a->list[0].p, cnt.cur(), th);
                });
            }
            // (launched for an empty interval as well: it zeroes the next round's counter)
            with_theta(a->theta, [&](auto C, auto th) {
                with_model(a->model, [&](auto D, auto model) {
                    hipLaunchKernelGGL((k_update_list<false, unsigned long long, true, decltype(D)::value, decltype(C)::value>),
                                       dim3(grid_for((size_t)std::max<long long>(gn, 1), 1024)), dim3(256), 0, ctx->stream, a->w[0].p,
                                       a->mask64.p, (long long*)nullptr, a->list[0].p, cnt.cur(), NoTab{}, a->active_v, cnt.next(), cur,
                                       model, th);
                });
            });
            NSOF_HIP(ctx, hipGetLastError());
            cnt.flip();
        }
        // the call's first frame has no predecessor to copy: one pass over the array
        if (k == 0 && (rc = accum_surface(a, which, cur))) return rc;
        a->slice_counter += every;
    }
    return NSOF_OK;
}

// Checkpoint / resume: the whole state of one array is w (float32 [H][W]), its refractory map (int64 [H][W],
// scheme 2) and the global slice counter that times the snapshots.
extern "C" int nsof_accum_read_state(nsof_accum* a, int which, float* w_out, int64_t* next_ok_out, int64_t* slice_counter)
{
    if (!a || which < 0 || which > (a->split ? 1 : 0)) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    if (w_out) NSOF_HIP(ctx, hipMemcpyAsync(w_out, a->w[which].p, a->npx * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (next_ok_out) {
        if (a->next_ok[which].p)
            NSOF_HIP(ctx, hipMemcpyAsync(next_ok_out, a->next_ok[which].p, a->npx * 8, hipMemcpyDeviceToHost, ctx->stream));
        else
            memset(next_ok_out, 0, a->npx * 8);
    }
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (slice_counter) *slice_counter = a->slice_counter;
    return NSOF_OK;
}

extern "C" int nsof_accum_write_state(nsof_accum* a, int which, const float* w_in, const int64_t* next_ok_in,
                                      int64_t slice_counter)
{
    if (!a || which < 0 || which > (a->split ? 1 : 0)) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    if (slice_counter < 0) return nsof_set_error(ctx, NSOF_EINVAL, "negative slice counter");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    if (w_in) NSOF_HIP(ctx, hipMemcpyAsync(a->w[which].p, w_in, a->npx * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (next_ok_in && a->next_ok[which].p)
        NSOF_HIP(ctx, hipMemcpyAsync(a->next_ok[which].p, next_ok_in, a->npx * 8, hipMemcpyHostToDevice, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    a->slice_counter = slice_counter;
    return NSOF_OK;
}

extern "C" int nsof_accum_update_state_p_dev(nsof_ctx* ctx, const nsof_accum_params* params, const float* d_w, const float* d_V,
                                             float* d_out, size_t n)
{
    if (!ctx || !d_w || !d_V || !d_out) return NSOF_EINVAL;
    Model model;
    if (int rc = model_of(ctx, params, &model)) return rc;
    if (!n) return NSOF_OK;
    nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
    hipLaunchKernelGGL(k_update_state, dim3(grid_for(n)), dim3(256), 0, ctx->stream, d_w, d_V, d_out, n, model.f);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_accum_update_state_dev(nsof_ctx* ctx, const float* d_w, const float* d_V, float* d_out, size_t n)
{
    return nsof_accum_update_state_p_dev(ctx, nullptr, d_w, d_V, d_out, n);
}

// Host arrays in, host histogram out (the reference calls it on the events of one slice).
extern "C" int nsof_accum_bincount_2d(nsof_ctx* ctx, const int16_t* x, const int16_t* y, size_t n, int height,
                                      int width, int32_t* counts_out)
{
    if (!ctx) return NSOF_EINVAL;
    if (!counts_out || (n && (!x || !y))) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
    if (height < 1 || width < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "empty sensor");
    for (size_t i = 0; i < n; i++)   // np.bincount raises on negative values; out-of-range ones would grow the array
        if (x[i] < 0 || y[i] < 0 || x[i] >= width || y[i] >= height)
            return nsof_set_error(ctx, NSOF_EINVAL, "event %zu (%d,%d) outside the %dx%d sensor", i, (int)x[i],
                                  (int)y[i], width, height);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)height * width;
    const size_t szE = (n * 2 + 255) & ~(size_t)255, szC = (npx * 4 + 255) & ~(size_t)255;
    int rc = ctx->stage.reserve(ctx, 2 * szE + szC);
    if (rc) return rc;
    short* dx = (short*)ctx->stage.p;
    short* dy = (short*)((char*)ctx->stage.p + szE);
    int* dc = (int*)((char*)ctx->stage.p + 2 * szE);
    NSOF_HIP(ctx, hipMemsetAsync(dc, 0, npx * 4, ctx->stream));
    if (n) {
        NSOF_HIP(ctx, hipMemcpyAsync(dx, x, n * 2, hipMemcpyHostToDevice, ctx->stream));
        NSOF_HIP(ctx, hipMemcpyAsync(dy, y, n * 2, hipMemcpyHostToDevice, ctx->stream));
        nsof_prof_scope ps(ctx, NSOF_K_ACCUM);
        hipLaunchKernelGGL(k_bincount, dim3(grid_for(n)), dim3(256), 0, ctx->stream, dx, dy, n, width, dc);
    }
    NSOF_HIP(ctx, hipGetLastError());
    NSOF_HIP(ctx, hipMemcpyAsync(counts_out, dc, npx * 4, hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NSOF_OK;
}

extern "C" int nsof_accum_resistance_p_dev(nsof_ctx* ctx, const nsof_accum_params* params, const float* d_w, float* d_out, size_t n)
{
    if (!ctx || !d_w || !d_out) return NSOF_EINVAL;
    Model model;
    if (int rc = model_of(ctx, params, &model)) return rc;
    if (!n) return NSOF_OK;
    hipLaunchKernelGGL(k_resistance<DevF>, dim3(grid_for(n)), dim3(256), 0, ctx->stream, d_w, d_out, n, model.f);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_accum_resistance_dev(nsof_ctx* ctx, const float* d_w, float* d_out, size_t n)
{
    return nsof_accum_resistance_p_dev(ctx, nullptr, d_w, d_out, n);
}

extern "C" int nsof_accum_read_w(nsof_accum* a, int which, float* out)
{
    if (!a || !out || which < 0 || which > (a->split ? 1 : 0)) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    NSOF_HIP(ctx, hipMemcpyAsync(out, a->w[which].p, a->npx * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NSOF_OK;
}

extern "C" int nsof_accum_read_resistance(nsof_accum* a, int which, float* out)
{
    if (!a || !out || which < 0 || which > (a->split ? 1 : 0)) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    nsof_dev_buf<float> tmp;
    int rc = tmp.reserve(ctx, a->npx * sizeof(float));
    if (rc) return rc;
    with_res(a->model, [&](auto res) {
        hipLaunchKernelGGL(k_resistance<decltype(res)>, dim3(grid_for(a->npx)), dim3(256), 0, ctx->stream, a->w[which].p, tmp.p, a->npx, res);
    });
    if (hipGetLastError() != hipSuccess) rc = nsof_set_error(ctx, NSOF_EDEVICE, "resistance launch failed");
    if (!rc) {
        hipError_t e = hipMemcpyAsync(out, tmp.p, a->npx * sizeof(float), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = nsof_set_error(ctx, NSOF_EDEVICE, "copy failed: %s", hipGetErrorString(e));
    }
    return rc;
}

extern "C" int64_t nsof_accum_snapshot_count(const nsof_accum* a) { return a ? a->snap_count : 0; }

// Block maximum of the device current (k_block_min_resistance) of the current state (snapshot < 0) or of a stored snapshot.
extern "C" int nsof_accum_block_current(nsof_accum* a, int which, int64_t snapshot, int memsize, double v_ds, double* out)
{
    if (!a || !out || which < 0 || which > (a->split ? 1 : 0) || memsize < 1 || memsize > a->W || memsize > a->H || !(v_ds > 0))
        return NSOF_EINVAL;
    if (snapshot >= a->snap_count) return nsof_set_error(a->ctx, NSOF_EINVAL, "snapshot %lld of %lld", (long long)snapshot, (long long)a->snap_count);
    nsof_ctx* ctx = a->ctx;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const int rows = a->H / memsize, cols = a->W / memsize;
    const size_t bytes = sizeof(double) * rows * cols;
    int rc = ctx->tmp.reserve(ctx, bytes);
    if (rc) return rc;
    const float* src = snapshot < 0 ? a->w[which].p : a->snap[which].p + (size_t)snapshot * a->npx;
    with_res(a->model, [&](auto res) {
        hipLaunchKernelGGL(k_block_min_resistance<decltype(res)>, dim3(cols, rows), dim3(256), 0, ctx->stream, src,
                           snapshot < 0 ? 1 : 0, a->W, memsize, cols, res, v_ds, (double*)ctx->tmp.p, (size_t)0, (size_t)0);
    });
    NSOF_HIP(ctx, hipGetLastError());
    NSOF_HIP(ctx, hipMemcpyAsync(out, ctx->tmp.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return NSOF_OK;
}

// Device twin: the map goes to DEVICE memory (d_out, rows x cols doubles), nothing is synchronised -- the input of
// nsof_roi_from_surface_dev, so that events -> surface -> ROI rectangles never visits the host.
extern "C" int nsof_accum_block_current_dev(nsof_accum* a, int which, int64_t snapshot, int memsize, double v_ds, double* d_out)
{
    if (!a || !d_out || which < 0 || which > (a->split ? 1 : 0) || memsize < 1 || memsize > a->W || memsize > a->H || !(v_ds > 0))
        return NSOF_EINVAL;
    if (snapshot >= a->snap_count) return nsof_set_error(a->ctx, NSOF_EINVAL, "snapshot %lld of %lld", (long long)snapshot, (long long)a->snap_count);
    nsof_ctx* ctx = a->ctx;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const int rows = a->H / memsize, cols = a->W / memsize;
    const float* src = snapshot < 0 ? a->w[which].p : a->snap[which].p + (size_t)snapshot * a->npx;
    with_res(a->model, [&](auto res) {
        hipLaunchKernelGGL(k_block_min_resistance<decltype(res)>, dim3(cols, rows), dim3(256), 0, ctx->stream, src,
                           snapshot < 0 ? 1 : 0, a->W, memsize, cols, res, v_ds, d_out, (size_t)0, (size_t)0);
    });
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_accum_read_snapshots(nsof_accum* a, int which, float* out, int64_t max_count)
{
    if (!a || which < 0 || which > (a->split ? 1 : 0)) return NSOF_EINVAL;
    nsof_ctx* ctx = a->ctx;
    const int64_t n = a->snap_count < max_count ? a->snap_count : max_count;
    if (n > 0) {
        if (!out) return NSOF_EINVAL;
        NSOF_HIP(ctx, hipMemcpyAsync(out, a->snap[which].p, (size_t)n * a->npx * sizeof(float), hipMemcpyDeviceToHost,
                                     ctx->stream));
        NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (which == (a->split ? 1 : 0)) a->snap_count = 0;  // cleared after the last array has been read
    return NSOF_OK;
}

extern "C" int64_t nsof_accum_slice_bounds(const int64_t* t, int64_t n, int64_t slice_us, int64_t* idx, int64_t cap)
{
    if (!t || n <= 0 || slice_us <= 0) return 0;
    const int64_t start = t[0], stop = t[n - 1] + slice_us;
    int64_t nb = (stop - start + slice_us - 1) / slice_us;
    if (nb < 0) nb = 0;
    if (idx) {
        int64_t pos = 0;
        for (int64_t i = 0; i < nb && i < cap; i++) {
            const int64_t b = start + i * slice_us;
            while (pos < n && t[pos] < b) pos++;
            idx[i] = pos;
        }
    }
    return nb;
}

// Bound i of a sorted DEVICE timestamp array: the first index with t >= t[0] + i * slice_us, a binary search -- on a sorted
// array what the scan above returns.  The two ends of t are the record's (k_stream_check, ORDER), so the number of bounds
// is formed here as the host forms it; one thread per bound below cap.
__global__ __launch_bounds__(256) static void k_slice_table(const long long* __restrict__ t, long long n, long long slice_us,
                                                             const unsigned long long* __restrict__ rec, long long* __restrict__ idx,
                                                             long long cap)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long start = (long long)rec[1], stop = (long long)rec[2] + slice_us;
    const long long nb = (stop - start + slice_us - 1) / slice_us;
    if (i >= cap || i >= nb) return;
    const long long b = start + i * slice_us;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (t[mid] < b) lo = mid + 1; else hi = mid;
    }
    idx[i] = lo;
}

extern "C" int64_t nsof_accum_slice_bounds_dev(nsof_ctx* ctx, const int64_t* d_t, int64_t n, int64_t slice_us, int64_t* idx, int64_t cap)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_t || n <= 0 || slice_us <= 0) return 0;
    const int64_t m = idx && cap > 0 ? cap : 0;
    if (m >= (1ll << 31)) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "slice_bounds: room for %lld bounds, 2^31 or more", (long long)m);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = stream_words(ctx, STREAM_REC + (size_t)m)) return rc;
    long long *const h = ctx->evtab_h.p, *const d = ctx->evtab.p;
    unsigned long long* const rec = reinterpret_cast<unsigned long long*>(d);
    NSOF_HIP(ctx, hipMemsetAsync(d, 0xFF, 8, ctx->stream));
    hipLaunchKernelGGL((k_stream_check<false, true>), dim3(grid_for((size_t)n)), dim3(256), 0, ctx->stream, (const short*)nullptr,
                       (const short*)nullptr, (const long long*)d_t, 0ll, (long long)n, 0, 0, rec);
    // the table is formed before the verdict is known: a search reads inside t whatever its order
    if (m)
        hipLaunchKernelGGL(k_slice_table, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, (const long long*)d_t, (long long)n,
                           (long long)slice_us, (const unsigned long long*)rec, d + STREAM_REC, (long long)m);
    NSOF_HIP(ctx, hipGetLastError());
    NSOF_HIP(ctx, hipMemcpyAsync(h, d, (STREAM_REC + (size_t)m) * 8, hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if ((unsigned long long)h[0] != STREAM_CLEAN)
        return nsof_set_error(ctx, NSOF_EINVAL, "slice_bounds: t is not non-decreasing: t[%lld] < t[%lld]", h[0], h[0] - 1);
    const int64_t start = h[1], stop = h[2] + slice_us;
    int64_t nb = (stop - start + slice_us - 1) / slice_us;
    if (nb < 0) nb = 0;
    if (m) memcpy(idx, h + STREAM_REC, (size_t)std::min(nb, m) * 8);
    return nb;
}
