// Statistics of an ensemble of flow fields against a reference flow (nsof_flow_ensemble_dev): the reduction of the
// Monte-Carlo device trials' flows of one frame pair (nsof/flowstats.py, pipeline.events_flow_variability_dev) into
// per-pixel moments of the deviation from the nominal flow and per-(trial, field) end-point-error figures, in one
// streaming pass over the trials' fields.
//
//   k_flow_ensemble         a lane owns FE_PX neighbouring pixels of one row of one field for the whole trial loop: their
//                           reference (u, v) and the running state (sum 2, sq 3, max 1 doubles per pixel) stay in
//                           registers, the trials' (u, v) are read FE_INFLIGHT trials at a time (the loads of a batch are
//                           issued before the first is consumed), and the state is written once at the end.  Per trial
//                           the wave adds its lanes' sqrt(e2) by a butterfly, counts the outliers and non-finite pixels
//                           from ballots, and the workgroup's first FE_INFLIGHT threads add the four waves' values in
//                           wave order into the workgroup's partial of that (trial, field).
//   k_flow_ensemble_finish  one workgroup per (trial, field) stages the workgroups' partials in LDS, one thread adds them
//                           in index order and divides.
//
// Arithmetic: double, every operation rounded on its own (the unit is compiled with
// -ffp-contract=off), trials in index order per pixel, so a run cut into chunks of trials with accumulate = 1 equals the
// one-shot run bit for bit.  The order of the pixel sum of aee -- butterfly over the 64 lanes (each lane: pixel 0 + pixel
// 1), waves 0..3, workgroups in index order (y-major) -- depends on the image size alone, neither on the trial count
// nor on how the trials are chunked, and holds no float atomics: aee has the same bits from run to run.  Lanes outside
// the image add +0.0.
#include <cmath>

#include "nsof_internal.h"

namespace {

// The tile of a workgroup (4 waves; wave w takes row FE_BY * blockIdx.y + w).  tests/test_flow_ensemble_cpu.py reads these.
constexpr int FE_PX = 2;         // neighbouring pixels per lane: one 16-byte load per trial when the rows allow it
constexpr int FE_BX = 128;       // pixels per workgroup along x = 64 lanes * FE_PX
constexpr int FE_BY = 4;         // rows per workgroup = waves per workgroup
constexpr int FE_INFLIGHT = 4;   // trials whose loads are issued before the first of them is consumed

struct Px {
    double su, sv, quu, qvv, quv, m;   // sum du, dv; sum du*du, dv*dv, du*dv; max of du*du + dv*dv
    double ru, rv;                     // the reference (u, v)
};

// One trial's (u, v) of one pixel into its state; returns e2.
__device__ __forceinline__ double fold(Px& s, float u, float v)
{
    const double du = (double)u - s.ru, dv = (double)v - s.rv;
    const double uu = du * du, vv = dv * dv;
    s.su += du;
    s.sv += dv;
    s.quu += uu;
    s.qvv += vv;
    s.quv += du * dv;
    const double e2 = uu + vv;
    if (e2 > s.m) s.m = e2;   // a NaN never enters, +inf does
    return e2;
}

// How a lane reads its pixel pair.  No load is predicated and every address is clamped into the image (a lane outside
// the image reads pixels of it and leaves them unused), so that the loads of a batch of trials are issued back to back.
enum fe_load {
    FE_LOAD_PX,       // two 8-byte loads, pixels min(x0, w - 1) and min(x0 + 1, w - 1)
    FE_LOAD_PAIR,     // one 16-byte load: every pair starts 16-byte aligned in every field, w even
    FE_LOAD_PAIR_ODD  // the same for an odd w >= 3: the lane of the last pixel reads pair 0 for nothing, and every lane adds an
                      // 8-byte load of pixel min(x0, w - 1)
};

struct fe_lane {
    bool in0, in1;          // the lane's two pixels lie in the image
    const float *pa, *pb;   // where trial 0 has (FE_LOAD_PX) pixel A and pixel B, (FE_LOAD_PAIR*) the pair and pixel A
    bool last;              // FE_LOAD_PAIR_ODD: pixel A is the row's last pixel, outside any whole pair
};

template <int LOAD>
__device__ __forceinline__ float4 load_pair(const fe_lane& l, ptrdiff_t off)
{
    if (LOAD == FE_LOAD_PX) {
        const float2 a = *reinterpret_cast<const float2*>(l.pa + off), b = *reinterpret_cast<const float2*>(l.pb + off);
        return make_float4(a.x, a.y, b.x, b.y);
    }
    float4 v = *reinterpret_cast<const float4*>(l.pa + off);
    if (LOAD == FE_LOAD_PAIR_ODD) {
        const float2 a = *reinterpret_cast<const float2*>(l.pb + off);
        v.x = l.last ? a.x : v.x;
        v.y = l.last ? a.y : v.y;
    }
    return v;
}

// The loads of N consecutive trials from t0 on.
template <int LOAD, int N>
__device__ __forceinline__ void load_batch(const fe_lane& l, int t0, ptrdiff_t ts, float4 (&v)[N])
{
#pragma unroll
    for (int j = 0; j < N; j++) v[j] = load_pair<LOAD>(l, (ptrdiff_t)(t0 + j) * ts);
}

// N consecutive trials from t0 on, loaded into v: trial by trial the fold, the wave's sums and counts into set `set` of
// the LDS slots; after the barrier the workgroup's first N threads write the partials of the N (trial, field)s.
template <int N>
__device__ __forceinline__ void fold_batch(const fe_lane& l, Px (&s)[FE_PX], const float4 (&v)[N], int t0, double tau2,
                                           double (&sh_e)[2][FE_INFLIGHT][4], int2 (&sh_n)[2][FE_INFLIGHT][4], int set,
                                           size_t part_at, double* __restrict__ part_e, int2* __restrict__ part_n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double inf = __builtin_huge_val();
#pragma unroll
    for (int j = 0; j < N; j++) {
        const double e2a = fold(s[0], v[j].x, v[j].y), e2b = fold(s[1], v[j].z, v[j].w);
        double e = (l.in0 ? sqrt(e2a) : 0.0) + (l.in1 ? sqrt(e2b) : 0.0);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) e += __shfl_xor(e, o, 64);
        const int outl = __popcll(__ballot(l.in0 && e2a > tau2)) + __popcll(__ballot(l.in1 && e2b > tau2));
        const int nonf = __popcll(__ballot(l.in0 && !(e2a < inf))) + __popcll(__ballot(l.in1 && !(e2b < inf)));
        if (lane == 0) {
            sh_e[set][j][wave] = e;
            sh_n[set][j][wave] = make_int2(outl, nonf);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < N) {
        const int j = threadIdx.x;
        const double e = ((sh_e[set][j][0] + sh_e[set][j][1]) + sh_e[set][j][2]) + sh_e[set][j][3];
        const int2 a = sh_n[set][j][0], b = sh_n[set][j][1], c = sh_n[set][j][2], d = sh_n[set][j][3];
        const size_t at = part_at + (size_t)(t0 + j) * gridDim.z * gridDim.y * gridDim.x;
        part_e[at] = e;
        part_n[at] = make_int2(a.x + b.x + c.x + d.x, a.y + b.y + c.y + d.y);
    }
}

template <int LOAD>
__global__ __launch_bounds__(256) void k_flow_ensemble(int n_trials, const float* __restrict__ flows, ptrdiff_t rs,
                                                       ptrdiff_t fs, ptrdiff_t ts, int w, int h,
                                                       const float* __restrict__ ref, ptrdiff_t rrs, ptrdiff_t rfs,
                                                       double tau2, int accumulate, double* __restrict__ sum,
                                                       double* __restrict__ sq, double* __restrict__ emax,
                                                       double* __restrict__ part_e, int2* __restrict__ part_n)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, f = blockIdx.z;
    const int x0 = (blockIdx.x * 64 + lane) * FE_PX, y = blockIdx.y * FE_BY + wave;
    const int xa = min(x0, w - 1), xb = min(x0 + 1, w - 1), yc = min(y, h - 1);
    fe_lane l;
    l.in0 = y < h && x0 < w;
    l.in1 = y < h && x0 + 1 < w;
    l.last = x0 == w - 1;
    const float* row = flows + (ptrdiff_t)f * fs + (ptrdiff_t)yc * rs;
    l.pa = row + 2 * (LOAD == FE_LOAD_PX ? xa : (x0 + 1 < w ? x0 : 0));
    l.pb = row + 2 * (LOAD == FE_LOAD_PX ? xb : xa);
    const size_t px = ((size_t)f * h + yc) * w + xa;   // the first pixel's index in the state arrays (used when in0)

    Px s[FE_PX] = {};
    if (ref && l.in0) {
        const float* r = ref + (ptrdiff_t)f * rfs + (ptrdiff_t)y * rrs + 2 * x0;
        s[0].ru = r[0];
        s[0].rv = r[1];
        if (l.in1) {
            s[1].ru = r[2];
            s[1].rv = r[3];
        }
    }
    if (accumulate) {
#pragma unroll
        for (int j = 0; j < FE_PX; j++)
            if (j ? l.in1 : l.in0) {
                s[j].su = sum[2 * (px + j)];
                s[j].sv = sum[2 * (px + j) + 1];
                s[j].quu = sq[3 * (px + j)];
                s[j].qvv = sq[3 * (px + j) + 1];
                s[j].quv = sq[3 * (px + j) + 2];
                s[j].m = emax[px + j];
            }
    }

    // the four waves' values of the trials of a batch; two sets, used in turn, so that one barrier per batch is enough
    __shared__ double sh_e[2][FE_INFLIGHT][4];
    __shared__ int2 sh_n[2][FE_INFLIGHT][4];
    // the partial of workgroup g (y-major) for (trial t, field f) is at (t * n_fields + f) * n_wg + g
    const size_t part_at = ((size_t)f * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    int t0 = 0, set = 0;
    for (; t0 + FE_INFLIGHT <= n_trials; t0 += FE_INFLIGHT, set ^= 1) {
        float4 v[FE_INFLIGHT];
        load_batch<LOAD>(l, t0, ts, v);
        fold_batch(l, s, v, t0, tau2, sh_e, sh_n, set, part_at, part_e, part_n);
    }
    for (; t0 < n_trials; t0++, set ^= 1) {   // the tail, a trial at a time
        float4 one[1];
        load_batch<LOAD>(l, t0, ts, one);
        fold_batch(l, s, one, t0, tau2, sh_e, sh_n, set, part_at, part_e, part_n);
    }

#pragma unroll
    for (int j = 0; j < FE_PX; j++)
        if (j ? l.in1 : l.in0) {
            sum[2 * (px + j)] = s[j].su;
            sum[2 * (px + j) + 1] = s[j].sv;
            sq[3 * (px + j)] = s[j].quu;
            sq[3 * (px + j) + 1] = s[j].qvv;
            sq[3 * (px + j) + 2] = s[j].quv;
            emax[px + j] = s[j].m;
        }
}

// aee, outliers, nonfinite of (trial, field) blockIdx.x from its n_wg workgroup partials.  The sum of the doubles is ONE
// chain in index order, so only its loads can be spread: the workgroup stages FE_FINISH_CHUNK partials at a time in LDS
// (every load of a chunk in flight at once) and thread 0 adds them in order; the integer counts have no order to keep.
constexpr int FE_FINISH_CHUNK = 2048;
__global__ __launch_bounds__(256) void k_flow_ensemble_finish(size_t n_wg, double pixels, const double* __restrict__ part_e,
                                                              const int2* __restrict__ part_n, double* __restrict__ aee,
                                                              int32_t* __restrict__ outliers, int32_t* __restrict__ nonfinite)
{
    __shared__ double sh[FE_FINISH_CHUNK];
    __shared__ int sh_n[2];
    const size_t tf = blockIdx.x;
    const double* pe = part_e + tf * n_wg;
    const int2* pn = part_n + tf * n_wg;
    if (threadIdx.x < 2) sh_n[threadIdx.x] = 0;
    double e = 0.0;
    int outl = 0, nonf = 0;
    for (size_t base = 0; base < n_wg; base += FE_FINISH_CHUNK) {
        const int n = (int)min((size_t)FE_FINISH_CHUNK, n_wg - base);
        double v[FE_FINISH_CHUNK / 256];
        int2 c[FE_FINISH_CHUNK / 256];
#pragma unroll
        for (int k = 0; k < FE_FINISH_CHUNK / 256; k++) {   // unpredicated, clamped: all of a thread's loads are in flight at once
            const int i = min((int)threadIdx.x + 256 * k, n - 1);
            v[k] = pe[base + i];
            c[k] = pn[base + i];
        }
#pragma unroll
        for (int k = 0; k < FE_FINISH_CHUNK / 256; k++) {
            const int i = threadIdx.x + 256 * k;
            if (i < n) {
                sh[i] = v[k];
                outl += c[k].x;
                nonf += c[k].y;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
#pragma unroll 8
            for (int i = 0; i < n; i++) e += sh[i];
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        outl += __shfl_xor(outl, o, 64);
        nonf += __shfl_xor(nonf, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&sh_n[0], outl);
        atomicAdd(&sh_n[1], nonf);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        aee[tf] = e / pixels;
        outliers[tf] = sh_n[0];
        nonfinite[tf] = sh_n[1];
    }
}

}  // namespace

extern "C" int nsof_flow_ensemble_dev(nsof_ctx* ctx, int n_trials, int n_fields, const float* d_flows,
                                      ptrdiff_t row_stride_floats, ptrdiff_t field_stride_floats,
                                      ptrdiff_t trial_stride_floats, int width, int height, const float* d_ref,
                                      ptrdiff_t ref_row_stride_floats, ptrdiff_t ref_field_stride_floats, double tau,
                                      int accumulate, double* d_sum, double* d_sq, double* d_epe2_max, double* d_aee,
                                      int32_t* d_outliers, int32_t* d_nonfinite)
{
    if (!ctx) return NSOF_EINVAL;
    if (n_trials < 1 || n_fields < 1 || width < 1 || height < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: n_trials %d, n_fields %d, size %dx%d", n_trials, n_fields,
                              width, height);
    if (!d_flows || !d_sum || !d_sq || !d_epe2_max || !d_aee || !d_outliers || !d_nonfinite)
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: null pointer (%s)",
                              !d_flows ? "d_flows" : !d_sum ? "d_sum" : !d_sq ? "d_sq" : !d_epe2_max ? "d_epe2_max"
                              : !d_aee ? "d_aee" : !d_outliers ? "d_outliers" : "d_nonfinite");
    if (row_stride_floats % 2 || row_stride_floats < 2 * (ptrdiff_t)width)
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: row stride %lld floats is odd or shorter than a row of %d pixels",
                              (long long)row_stride_floats, width);
    if ((reinterpret_cast<uintptr_t>(d_flows) & 7) || (n_fields > 1 && field_stride_floats % 2) || (n_trials > 1 && trial_stride_floats % 2))
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: flows at %p with field stride %lld, trial stride %lld floats are not "
                              "8-byte aligned", (const void*)d_flows, (long long)field_stride_floats, (long long)trial_stride_floats);
    if (d_ref && (ref_row_stride_floats % 2 || ref_row_stride_floats < 2 * (ptrdiff_t)width))
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: reference row stride %lld floats is odd or shorter than a row of "
                              "%d pixels", (long long)ref_row_stride_floats, width);
    if (d_ref && ((reinterpret_cast<uintptr_t>(d_ref) & 7) || (n_fields > 1 && ref_field_stride_floats % 2)))
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: reference at %p with field stride %lld floats is not 8-byte aligned",
                              (const void*)d_ref, (long long)ref_field_stride_floats);
    if (accumulate != 0 && accumulate != 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: accumulate %d is neither 0 nor 1", accumulate);
    if (!(tau >= 0)) return nsof_set_error(ctx, NSOF_EINVAL, "flow_ensemble: tau %g is negative or NaN", tau);
    if ((long long)width * height > (1ll << 27))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "flow_ensemble: %dx%d is more than 2^27 pixels", width, height);
    const dim3 grid((width + FE_BX - 1) / FE_BX, (height + FE_BY - 1) / FE_BY, n_fields);
    const size_t n_wg = (size_t)grid.x * grid.y, n_tf = (size_t)n_trials * n_fields;
    if (grid.y > 65535 || n_fields > 65535 || n_tf > 0x7fffffffull || n_wg * n_tf > (1ull << 40))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "flow_ensemble: %d trials of %d fields of %dx%d are beyond one launch",
                              n_trials, n_fields, width, height);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    // the workgroups' partials: n_wg * n_tf doubles, then as many int2
    int rc = ctx->tmp.reserve(ctx, n_wg * n_tf * (sizeof(double) + sizeof(int2)));
    if (rc) return rc;
    double* part_e = (double*)ctx->tmp.p;
    int2* part_n = (int2*)(part_e + n_wg * n_tf);
    const bool pairs = width >= 2 && (reinterpret_cast<uintptr_t>(d_flows) & 15) == 0 && row_stride_floats % 4 == 0 &&
                       (n_fields == 1 || field_stride_floats % 4 == 0) && (n_trials == 1 || trial_stride_floats % 4 == 0);
    const double tau2 = tau * tau;
    auto launch = [&](auto load) {
        hipLaunchKernelGGL(k_flow_ensemble<decltype(load)::value>, grid, dim3(256), 0, ctx->stream, n_trials, d_flows,
                           row_stride_floats, field_stride_floats, trial_stride_floats, width, height, d_ref,
                           ref_row_stride_floats, ref_field_stride_floats, tau2, accumulate, d_sum, d_sq, d_epe2_max, part_e,
                           part_n);
    };
    nsof_with_int<FE_LOAD_PX, FE_LOAD_PAIR_ODD>(!pairs ? FE_LOAD_PX : width % 2 ? FE_LOAD_PAIR_ODD : FE_LOAD_PAIR, launch);
    NSOF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_flow_ensemble_finish, dim3((unsigned)n_tf), dim3(256), 0, ctx->stream, n_wg,
                       (double)((long long)width * height), part_e, part_n, d_aee, d_outliers, d_nonfinite);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
