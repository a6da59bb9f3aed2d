// Frame-driven synaptic accumulator, float64: simulate_memristor_array of
// /root/reference/simulation/simulationcode_v4_transistor_uav.m (:146-227, 332-347) for gfx950.
//
// One kernel, one launch site, one host path.  k_frames_run walks every frame pair of one (trial, cell) in one thread -- a
// cell's pairs are one dependent chain, the cells and the trials are independent -- and is instantiated per SOURCE of the
// device model: the fitted constants, one device in the kernel arguments, or planes with a value per (trial, cell).  The
// source is read once, before the loop; the loop itself exists once.  nsof_accum_frames_f64_c2c_dev is the only function
// that launches it and nsof_accum_frames_f64_c2c the only one that copies; the other six entries forward to them.
// Cycle-to-cycle write noise is a second template argument of the same kernel (NOISE): one factor per frame pair from the
// counter generator of accum_c2c.h; a call without noise launches the NOISE = false instantiations, the kernel as it was.
// The bits of the run -- the default device, two other devices, the dead zone -- are recorded in
// tests/golden/frames_run_bits.npz, written by the per-pair host entry this file replaced (tests/test_frames_bits_gpu.py).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#include "accum_c2c.h"
#include "accum_model.h"

namespace {

// update_state(w, V, dt, params) of the script (:173-181): k * A^alpha * B^b, left to right; alpha == 1 calls no pow.
__device__ __forceinline__ double frame_gain(double V, double v0, double k, double alpha)
{
    const double a = V / v0 - 1;
    return k * (alpha == 1.0 ? a : pow(a, alpha));
}
//   NOISE  the step scaled by the pair's write-noise factor: nw = w + (dwdt * f) * dt, each operation rounded on its own
template <bool NOISE>
__device__ __forceinline__ double frame_update(double w, double V, double dt, const DevD& p, [[maybe_unused]] double f)
{
    double dwdt = 0.0;
    if (V < p.voff) dwdt = frame_gain(V, p.voff, p.koff, p.alphaoff) * pow(1 - w * p.soff, p.boff);
    else if (V > p.von) dwdt = frame_gain(V, p.von, p.kon, p.alphaon) * pow(1 - w * p.son, p.bon);
    if constexpr (NOISE) dwdt = dwdt * f;
    const double nw = w + dwdt * dt;
    return nw < 0 ? 0 : (nw > 1 ? 1 : nw);
}

// Cycle-to-cycle write noise of the run (nsof_accum_frames_f64_c2c_dev): what a NOISE arm is handed.  A "cycle" is one
// write, one frame pair: the factor is drawn once per pair and held for its n_sub sub-steps, which are the Euler
// integration of that one pulse.  The frame path is array 0 of the counter layout, its slice the absolute pair index.
struct FrameC2c {
    unsigned k0, k1;           // the seed's two words
    float sigma_off, sigma_on;
    long long first_pair;      // the absolute index of the call's first pair
};
struct NoFrameC2c {};
template <bool NOISE>
using FrameC2cArg = std::conditional_t<NOISE, FrameC2c, NoFrameC2c>;   // no noise passes nothing

// f = max(0, 1 + sigma * xi) of pair q of (trial, cell), sigma that of the branch V takes at the cell's own thresholds; the
// float product is exact in double, the sum is rounded once.  The dead zone, or a branch whose sigma is 0: 1.0 and no draw
// (dwdt * 1.0 is dwdt).  A pulse may fail to switch, it never switches backwards.
__device__ __forceinline__ double frame_c2c_factor(const FrameC2c& nz, double V, const DevD& p, unsigned cell, long long q,
                                                   unsigned trial)
{
    const float sigma = V < p.voff ? nz.sigma_off : (V > p.von ? nz.sigma_on : 0.f);
    if (sigma == 0.f) return 1.0;
    const float xi = c2c_xi(nz.k0, nz.k1, cell, (unsigned long long)q, c2c_trial_word(0, (int)trial));
    const double u = 1.0 + (double)sigma * (double)xi;
    return u < 0 ? 0.0 : u;
}

// One frame pair of one grid pixel: the state after n_sub sub-steps under the drive voltage of |a - b|.
//   NOISE  pair q of (trial, cell): the factor is formed once, before the sub-step loop
template <bool NOISE>
__device__ __forceinline__ double frame_pair(double a, double b, double ww, double dts, int n_sub, double th1, double th2,
                                             const DevD& p, [[maybe_unused]] const FrameC2cArg<NOISE>& nz,
                                             [[maybe_unused]] unsigned cell, [[maybe_unused]] long long q,
                                             [[maybe_unused]] unsigned trial)
{
    const double d = fabs(a * 256 - b * 256);
    double V = d > th1 ? (d + 4) * 0.75 : (d - 5.5) * 0.6;   // func2 == func3 in the source
    V = V > 0 ? -(0.3 * V + 0) : (V < 0 ? -(3 * V + -3) : 0.0);
    double f = 1.0;
    if constexpr (NOISE) f = frame_c2c_factor(nz, V, p, cell, q, trial);
    for (int s = 0; s < n_sub; s++) ww = frame_update<NOISE>(ww, V, dts, p, f);
    return ww;
}

// The three sources of a thread's DevD, read through frame_cell(source, trial, cell):
//   FittedD    the fitted device: compile-time constants but for the two values the host forms with libm
//   DevD       one device in the kernel arguments, the same for every thread
//   FrameMaps  per field the scalar of the call or the thread's element of a plane [1 or n_trials][n] (trial stride 0: the
//              plane is shared by the trials); lambda and r0 are planes too wherever Ron, Roff or wini is one
struct FittedD { double lambda, r0; };
enum { FM_VOFF, FM_VON, FM_KOFF, FM_KON, FM_SON, FM_SOFF, FM_BON, FM_BOFF, FM_ALPHAOFF, FM_ALPHAON, FM_RON, FM_LAMBDA, FM_WINI, FM_R0, FM_COUNT };   // DevD's fields, in order
struct FrameMaps {
    const double* plane[FM_COUNT];   // nullptr: the field is the scalar
    size_t stride[FM_COUNT];         // between the trials of a plane: 0 or n
    double scalar[FM_COUNT];
};
__device__ __forceinline__ DevD frame_cell(const DevD& p, size_t, size_t) { return p; }
__device__ __forceinline__ DevD frame_cell(FittedD a, size_t, size_t)
{
    DevD p = fitted_d();
    p.lambda = a.lambda;
    p.r0 = a.r0;
    return p;
}
__device__ __forceinline__ DevD frame_cell(const FrameMaps& m, size_t trial, size_t i)
{
    auto get = [&](int s) { return m.plane[s] ? m.plane[s][trial * m.stride[s] + i] : m.scalar[s]; };
    return DevD{get(FM_VOFF), get(FM_VON), get(FM_KOFF), get(FM_KON), get(FM_SON), get(FM_SOFF), get(FM_BON), get(FM_BOFF),
                get(FM_ALPHAOFF), get(FM_ALPHAON), get(FM_RON), get(FM_LAMBDA), get(FM_WINI), get(FM_R0)};
}

// The whole run in one launch: thread g is trial g / n, cell g % n, and walks every frame pair.  imgs [n_frames][n] is
// shared by the trials; w [T][n]; res [T][n_frames][n] (optional), slice 0 = r0; current [T][n_frames - 1][n] = v_ds /
// res[f + 1] (optional).  total = T * n.
//   NOISE  cycle-to-cycle write noise: one factor per pair, formed before the sub-step loop; without it nz is empty and the
//          instantiation is the kernel as it was
template <class Src, bool NOISE>
__global__ __launch_bounds__(64) void k_frames_run(const double* __restrict__ imgs, int n_frames, double* __restrict__ w,
                                                    double* __restrict__ res, double* __restrict__ current, size_t n,
                                                    size_t total, double dts, int n_sub, double th1, double th2, Src src,
                                                    double v_ds, FrameC2cArg<NOISE> nz)
{
    const size_t g = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (g >= total) return;
    const size_t trial = g / n, i = g - trial * n;
    const DevD p = frame_cell(src, trial, i);
    double* const rt = res ? res + trial * (size_t)n_frames * n : nullptr;
    double* const ct = current ? current + trial * (size_t)(n_frames - 1) * n : nullptr;
    double ww = p.wini, b = imgs[i];
    if (rt) rt[i] = p.r0;
    for (int f = 0; f + 1 < n_frames; f++) {
        const double a = b;
        b = imgs[(size_t)(f + 1) * n + i];
        // (the noiseless arm names neither the cell nor the trial here: its code object is then the one it was, register for
        // register)
        if constexpr (NOISE) ww = frame_pair<true>(a, b, ww, dts, n_sub, th1, th2, p, nz, (unsigned)i, nz.first_pair + f, (unsigned)trial);
        else ww = frame_pair<false>(a, b, ww, dts, n_sub, th1, th2, p, nz, 0, 0, 0);
        const double r = p.ron / exp(-p.lambda * (1 - ww));
        if (rt) rt[(size_t)(f + 1) * n + i] = r;
        if (ct) ct[(size_t)f * n + i] = v_ds / r;
    }
    w[g] = ww;
}

// Everything that can refuse a frame-driven call, decided on the host before anything is uploaded, launched or written:
// the arguments, the launch range, the scalars (model_of) and every value of every plane against the same domain
// (key_value_refused) -- so a plane is refused exactly where the uniform entry refuses that scalar.
int frame_planes_of(nsof_ctx* ctx, int n_frames, int height, int width, int n_sub_steps, const nsof_accum_params* params,
                    int n_trials, int n_maps, const int* keys, const double* const* planes, const int* plane_trials, Model* model,
                    PlaneSet<double>* fp)
{
    if (n_frames < 1 || height < 1 || width < 1 || n_sub_steps < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "bad frame-accumulator arguments");
    if (int rc = model_of(ctx, params, model)) return rc;
    if (int rc = plane_set_of(ctx, PlaneLabels{"frame maps", "frame map"}, *model, height, width, n_trials, n_maps, keys, planes,
                              plane_trials, fp))
        return rc;
    const size_t npx = (size_t)height * width;
    if (npx > (0xffffffffull - 63) / (size_t)n_trials)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%d trials of %zu cells: too large for one launch", n_trials, npx);
    return NSOF_OK;
}

// ... and what the noise arguments can refuse, ahead of it.  *noise: some spread is non-zero, the NOISE arms run.
int frame_c2c_of(nsof_ctx* ctx, const nsof_accum_c2c* c2c, int64_t first_pair, int n_frames, int n_trials, bool* noise)
{
    *noise = false;
    if (c2c) {
        if (!(c2c->sigma_on >= 0.f) || !std::isfinite(c2c->sigma_on))
            return nsof_set_error(ctx, NSOF_EINVAL, "cycle-to-cycle noise: sigma_on = %g is not a finite number >= 0", (double)c2c->sigma_on);
        if (!(c2c->sigma_off >= 0.f) || !std::isfinite(c2c->sigma_off))
            return nsof_set_error(ctx, NSOF_EINVAL, "cycle-to-cycle noise: sigma_off = %g is not a finite number >= 0", (double)c2c->sigma_off);
        *noise = c2c->sigma_on != 0.f || c2c->sigma_off != 0.f;   // both 0: the noiseless kernels
    }
    if (first_pair < 0 || first_pair > INT64_MAX - std::max(n_frames, 0))
        return nsof_set_error(ctx, NSOF_EINVAL, "first_pair = %lld: a pair index >= 0 whose sum with the %d frames fits an int64",
                              (long long)first_pair, n_frames);
    if (*noise && n_trials > 65535)   // the trial shares its counter word with the array, as in the event-driven trial run
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "cycle-to-cycle noise: n_trials = %d, at most 65535 trials draw distinct variates",
                              n_trials);
    return NSOF_OK;
}

// The kernel's FrameMaps of a mapped call: one table -- the caller's planes, then lambda and r0 per (trial, cell) wherever
// Ron, Roff or wini is a plane, formed with the host's log / exp as model_of forms the two scalars -- through the pinned
// copy of the context, which waits for this entry's previous upload only (or to grow).
int frame_maps_upload(nsof_ctx* ctx, const Model& model, const PlaneSet<double>& fp, size_t npx, FrameMaps* fm)
{
    // slot -> key of nsof_accum_params (lambda and r0 have none)
    static const int key_of[FM_COUNT] = {NSOF_ACCUM_KEY_VOFF, NSOF_ACCUM_KEY_VON, NSOF_ACCUM_KEY_KOFF, NSOF_ACCUM_KEY_KON,
                                         NSOF_ACCUM_KEY_SON, NSOF_ACCUM_KEY_SOFF, NSOF_ACCUM_KEY_BON, NSOF_ACCUM_KEY_BOFF,
                                         NSOF_ACCUM_KEY_ALPHAOFF, NSOF_ACCUM_KEY_ALPHAON, NSOF_ACCUM_KEY_RON, -1,
                                         NSOF_ACCUM_KEY_WINI, -1};
    const DevD& md = model.d;
    const nsof_accum_params& sp = model.prm;
    const double scalars[FM_COUNT] = {md.voff, md.von, md.koff, md.kon, md.son, md.soff, md.bon, md.boff, md.alphaoff, md.alphaon,
                                      md.ron, md.lambda, md.wini, md.r0};
    const int t_lam = fp.lambda_trials(), t_r0 = std::max(t_lam, fp.trials[NSOF_ACCUM_KEY_WINI]);
    size_t off[FM_COUNT], doubles = 0;
    int trials[FM_COUNT];
    for (int s = 0; s < FM_COUNT; s++) {
        trials[s] = s == FM_LAMBDA ? t_lam : (s == FM_R0 ? t_r0 : fp.trials[key_of[s]]);
        off[s] = doubles;
        doubles += (size_t)trials[s] * npx;
    }
    const size_t bytes = doubles * sizeof(double);
    if (int rc = ctx->frame_maps.stage(ctx, bytes, (bytes + bytes / 2 + 4095) & ~(size_t)4095)) return rc;
    double* h = (double*)ctx->frame_maps.h.p;
    for (int s = 0; s < FM_COUNT; s++) {
        double* dst = h + off[s];
        const size_t cnt = (size_t)trials[s] * npx;
        if (s == FM_LAMBDA) {
            for (size_t e = 0; e < cnt; e++) dst[e] = fp.lambda_at(sp, e / npx, e % npx, npx);
        } else if (s == FM_R0) {
            for (size_t e = 0; e < cnt; e++) {
                const size_t t = e / npx, i = e % npx;
                const double lam = t_lam ? h[off[FM_LAMBDA] + (t_lam == 1 ? 0 : t) * npx + i] : md.lambda;
                dst[e] = fp.at(NSOF_ACCUM_KEY_RON, sp.Ron, t, i, npx) / std::exp(-lam * (1 - fp.at(NSOF_ACCUM_KEY_WINI, sp.wini, t, i, npx)));
            }
        } else if (cnt) {
            memcpy(dst, fp.plane[key_of[s]], cnt * sizeof(double));
        }
    }
    const double* d_planes = (const double*)ctx->frame_maps.upload(ctx, bytes);
    if (!d_planes) return NSOF_EDEVICE;
    for (int s = 0; s < FM_COUNT; s++) {
        fm->plane[s] = trials[s] ? d_planes + off[s] : nullptr;
        fm->stride[s] = trials[s] > 1 ? npx : 0;
        fm->scalar[s] = scalars[s];
    }
    return NSOF_OK;
}

}  // namespace

// The device entry every other one ends in: see include/nsof.h.
extern "C" int nsof_accum_frames_f64_c2c_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                                             int n_sub_steps, double th1, double th2, double v_ds, const nsof_accum_params* params,
                                             int n_trials, int n_maps, const int* keys, const double* const* planes,
                                             const int* plane_trials, double* d_w, double* d_res, double* d_current,
                                             const nsof_accum_c2c* c2c, int64_t first_pair)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_imgs || !d_w) return nsof_set_error(ctx, NSOF_EINVAL, "bad frame-accumulator arguments");
    bool noise;
    if (int rc = frame_c2c_of(ctx, c2c, first_pair, n_frames, n_trials, &noise)) return rc;
    Model model;
    PlaneSet<double> fp;
    if (int rc = frame_planes_of(ctx, n_frames, height, width, n_sub_steps, params, n_trials, n_maps, keys, planes, plane_trials,
                                 &model, &fp))
        return rc;
    const size_t npx = (size_t)height * width, total = npx * (size_t)n_trials;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    auto launch_arm = [&](auto src, auto N, auto nz) {
        hipLaunchKernelGGL((k_frames_run<decltype(src), decltype(N)::value>), dim3((unsigned)((total + 63) / 64)), dim3(64), 0,
                           ctx->stream, d_imgs, n_frames, d_w, d_res, d_current, npx, total, dt / n_sub_steps, n_sub_steps, th1, th2,
                           src, v_ds, nz);
    };
    auto launch = [&](auto src) {
        if (noise)
            launch_arm(src, std::true_type{},
                       FrameC2c{(unsigned)c2c->seed, (unsigned)(c2c->seed >> 32), c2c->sigma_off, c2c->sigma_on, (long long)first_pair});
        else
            launch_arm(src, std::false_type{}, NoFrameC2c{});
    };
    if (fp.any) {
        FrameMaps fm;
        if (int rc = frame_maps_upload(ctx, model, fp, npx, &fm)) return rc;
        launch(fm);
    } else if (model.fitted) {
        launch(FittedD{model.d.lambda, model.d.r0});
    } else {
        launch(model.d);
    }
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_accum_frames_f64_maps_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                                              int n_sub_steps, double th1, double th2, double v_ds, const nsof_accum_params* params,
                                              int n_trials, int n_maps, const int* keys, const double* const* planes,
                                              const int* plane_trials, double* d_w, double* d_res, double* d_current)
{
    return nsof_accum_frames_f64_c2c_dev(ctx, d_imgs, n_frames, height, width, dt, n_sub_steps, th1, th2, v_ds, params, n_trials, n_maps,
                                         keys, planes, plane_trials, d_w, d_res, d_current, nullptr, 0);
}

extern "C" int nsof_accum_frames_f64_p_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                                           int n_sub_steps, double th1, double th2, double v_ds, const nsof_accum_params* params,
                                           double* d_w, double* d_res, double* d_current)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_imgs || !d_w || !d_res || n_frames < 1 || height < 1 || width < 1 || n_sub_steps < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "bad frame-accumulator arguments");
    return nsof_accum_frames_f64_maps_dev(ctx, d_imgs, n_frames, height, width, dt, n_sub_steps, th1, th2, v_ds, params, 1, 0, nullptr,
                                          nullptr, nullptr, d_w, d_res, d_current);
}

extern "C" int nsof_accum_frames_f64_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                                         int n_sub_steps, double th1, double th2, double v_ds, double* d_w, double* d_res,
                                         double* d_current)
{
    return nsof_accum_frames_f64_p_dev(ctx, d_imgs, n_frames, height, width, dt, n_sub_steps, th1, th2, v_ds, nullptr, d_w, d_res,
                                       d_current);
}

// The host path: validate, upload the frames, the device entry, download, synchronise.
extern "C" int nsof_accum_frames_f64_c2c(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                                         int n_sub_steps, double th1, double th2, const nsof_accum_params* params, int n_trials,
                                         int n_maps, const int* keys, const double* const* planes, const int* plane_trials,
                                         double* w_out, double* res_out, const nsof_accum_c2c* c2c, int64_t first_pair)
{
    if (!ctx) return NSOF_EINVAL;
    if (!imgs || !w_out || !res_out) return nsof_set_error(ctx, NSOF_EINVAL, "bad frame-accumulator arguments");
    {   // refuse before anything is allocated or copied
        bool noise;
        if (int rc = frame_c2c_of(ctx, c2c, first_pair, n_frames, n_trials, &noise)) return rc;
        Model model;
        PlaneSet<double> fp;
        if (int rc = frame_planes_of(ctx, n_frames, height, width, n_sub_steps, params, n_trials, n_maps, keys, planes, plane_trials,
                                     &model, &fp))
            return rc;
    }
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t npx = (size_t)height * width, nw = npx * (size_t)n_trials, nr = nw * (size_t)n_frames;
    nsof_dev_buf<double> img_buf, w_buf, res_buf;
    int rc = img_buf.reserve(ctx, (size_t)n_frames * npx * 8);
    if (!rc) rc = w_buf.reserve(ctx, nw * 8);
    if (!rc) rc = res_buf.reserve(ctx, nr * 8);
    if (rc) return rc;
    NSOF_HIP(ctx, hipMemcpyAsync(img_buf.p, imgs, (size_t)n_frames * npx * 8, hipMemcpyHostToDevice, ctx->stream));
    rc = nsof_accum_frames_f64_c2c_dev(ctx, img_buf.p, n_frames, height, width, dt, n_sub_steps, th1, th2, 1.0, params, n_trials,
                                       n_maps, keys, planes, plane_trials, w_buf.p, res_buf.p, nullptr, c2c, first_pair);
    hipError_t e = hipSuccess;
    if (!rc) e = hipMemcpyAsync(w_out, w_buf.p, nw * 8, hipMemcpyDeviceToHost, ctx->stream);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(res_out, res_buf.p, nr * 8, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);   // also before the buffers go
    if (rc) return rc;
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return nsof_set_error(ctx, NSOF_EDEVICE, "frame accumulator: %s", hipGetErrorString(e));
    return NSOF_OK;
}

extern "C" int nsof_accum_frames_f64_maps(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                                          int n_sub_steps, double th1, double th2, const nsof_accum_params* params, int n_trials,
                                          int n_maps, const int* keys, const double* const* planes, const int* plane_trials,
                                          double* w_out, double* res_out)
{
    return nsof_accum_frames_f64_c2c(ctx, imgs, n_frames, height, width, dt, n_sub_steps, th1, th2, params, n_trials, n_maps, keys, planes,
                                     plane_trials, w_out, res_out, nullptr, 0);
}

extern "C" int nsof_accum_frames_f64_p(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                                       int n_sub_steps, double th1, double th2, const nsof_accum_params* params, double* w_out,
                                       double* res_out)
{
    return nsof_accum_frames_f64_maps(ctx, imgs, n_frames, height, width, dt, n_sub_steps, th1, th2, params, 1, 0, nullptr, nullptr,
                                      nullptr, w_out, res_out);
}

extern "C" int nsof_accum_frames_f64(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                                     int n_sub_steps, double th1, double th2, double* w_out, double* res_out)
{
    return nsof_accum_frames_f64_p(ctx, imgs, n_frames, height, width, dt, n_sub_steps, th1, th2, nullptr, w_out, res_out);
}
