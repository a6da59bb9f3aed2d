// Farneback dense optical flow, coarse-to-fine flow resample for gfx950 (CDNA4, wave64): resize(prevFlow, INTER_LINEAR)
// then "flow *= 1/pyr_scale".  Three kernels -- one thread per pixel (any sizes), a 2x2 block per thread and a row walk
// (both upsampling only) -- and their two launchers.  The pyramid levels are in farneback_pyramid.hip; the tap and blend
// helpers the two share (lin_tap_x / lin_tap_y, lin_mix, lin_blend) are in nsof_internal.h.
//
// Flow fields are [n][h][w][2] f32.  The kernels keep resize's operation order (horizontal blend, then vertical; see
// DESIGN.md "numerics contract"); this translation unit is compiled with -ffp-contract=off, and every blend is
// nsof_madd<FMA>: the launchers read the arithmetic variant from ctx->opt_pyr_fma (NSOF_OPT_PYR_FMA).
#include "nsof_internal.h"

namespace {

// Two adjacent flow vectors of a destination row: one streamed 16-B store where both exist and drow is 16-byte aligned
// (vec), else one or two 8-B stores.
__device__ __forceinline__ void store_flow_pair(float2* drow, const float2 (&o)[2], bool vec, bool second)
{
    if (vec) {
        const float f[4] = {o[0].x, o[0].y, o[1].x, o[1].y};
        nsof_store_stream_n(reinterpret_cast<float*>(drow), f);
    } else {
        drow[0] = o[0];
        if (second) drow[1] = o[1];
    }
}

template <bool FMA>
__global__ __launch_bounds__(256) void k_flow_upsample(const float* __restrict__ src, int sw, int sh,
                                                        float* __restrict__ dst, int dw, int dh, double scale_x,
                                                        double scale_y, float mul)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= dw || dy >= dh) return;
    const LinTap tx = lin_tap_x(dx, scale_x, sw), ty = lin_tap_y(dy, scale_y, sh);
    const float2* S = reinterpret_cast<const float2*>(src) + (size_t)blockIdx.z * sw * sh;
    const float2 p00 = S[(size_t)ty.i0 * sw + tx.i0], p01 = S[(size_t)ty.i0 * sw + tx.i1];
    const float2 p10 = S[(size_t)ty.i1 * sw + tx.i0], p11 = S[(size_t)ty.i1 * sw + tx.i1];
    const float2 o = lin_blend<FMA>(p00, p01, p10, p11, tx.w1, ty.w1);
    reinterpret_cast<float2*>(dst)[((size_t)blockIdx.z * dh + dy) * dw + dx] = make_float2(o.x * mul, o.y * mul);
}

// Upsampling variant: a thread produces a 2x2 block of destination pixels.  When dst >= src in both directions,
// consecutive destination coordinates map to source coordinates at most one apart, so the block's 4 pixels
// sample from a 3x3 source neighbourhood: 9 float2 loads + 2 float4 stores per 4 pixels instead of 16 + 4 (the L1
// serves 4 lanes per cycle per instruction, whatever its width).  Same arithmetic per pixel as k_flow_upsample.
// HET: field z is work item z of the device table (its sizes, its offsets into src / dst).
template <bool HET, bool FMA>
__global__ __launch_bounds__(256) void k_flow_upsample2x2(const float* __restrict__ src, int sw, int sh,
                                                           float* __restrict__ dst, int dw, int dh, double scale_x,
                                                           double scale_y, float mul,
                                                           const nsof_het_item* __restrict__ items)
{
    const int bx = blockIdx.x * 64 + (threadIdx.x & 63), by = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int dx0 = 2 * bx, dy0 = 2 * by;
    size_t s_off, d_off;   // float2 offsets of this field in src / dst
    if constexpr (HET) {
        const nsof_het_item& it = items[blockIdx.z];
        sw = it.pw; sh = it.ph; dw = it.wk; dh = it.hk;
        s_off = it.offFc;
        d_off = it.offF;
        if (dx0 >= dw || dy0 >= dh) return;
        if (sw == 0) {   // the item's coarsest level: its incoming flow is zero
            float2* D = reinterpret_cast<float2*>(dst) + d_off;
            for (int i = 0; i < 2 && dy0 + i < dh; i++)
                for (int j = 0; j < 2 && dx0 + j < dw; j++) D[(size_t)(dy0 + i) * dw + dx0 + j] = make_float2(0.f, 0.f);
            return;
        }
        scale_x = inv_scale(dw, sw);
        scale_y = inv_scale(dh, sh);
    } else {
        s_off = (size_t)blockIdx.z * sw * sh;
        d_off = (size_t)blockIdx.z * dw * dh;
        if (dx0 >= dw || dy0 >= dh) return;
    }
    LinTap tx[2];
    int sy[2];   // unclamped: the block's rows are sy[0] + {0, 1, 2}, clamped below
    float b1[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        tx[i] = lin_tap_x(min(dx0 + i, dw - 1), scale_x, sw);
        lin_coord_y(min(dy0 + i, dh - 1), scale_y, sy[i], b1[i]);
    }
    const float2* S = reinterpret_cast<const float2*>(src) + s_off;
    // source columns tx[0].i0 + {0,1,2} and rows sy[0] + {0,1,2}, clamped like the per-pixel kernel clamps them
    float2 v[3][3];
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const float2* row = S + (size_t)clampi(sy[0] + r, 0, sh - 1) * sw;
#pragma unroll
        for (int c = 0; c < 3; c++) v[r][c] = row[min(tx[0].i0 + c, sw - 1)];
    }
    float2* D = reinterpret_cast<float2*>(dst) + d_off;
#pragma unroll
    for (int i = 0; i < 2; i++) {          // destination row dy0 + i
        if (dy0 + i >= dh) break;
        const int ro = sy[i] - sy[0];       // 0 or 1
        float2 o[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {      // destination column dx0 + j
            const int co = tx[j].i0 - tx[0].i0;   // 0 or 1
            const float2 p00 = ro ? (co ? v[1][1] : v[1][0]) : (co ? v[0][1] : v[0][0]);
            const float2 p01 = ro ? (co ? v[1][2] : v[1][1]) : (co ? v[0][2] : v[0][1]);
            const float2 p10 = ro ? (co ? v[2][1] : v[2][0]) : (co ? v[1][1] : v[1][0]);
            const float2 p11 = ro ? (co ? v[2][2] : v[2][1]) : (co ? v[1][2] : v[1][1]);
            const float2 t = lin_blend<FMA>(p00, p01, p10, p11, tx[j].w1, b1[i]);
            o[j] = make_float2(t.x * mul, t.y * mul);
        }
        store_flow_pair(D + (size_t)(dy0 + i) * dw + dx0, o,
                        dx0 + 1 < dw && (dw & 1) == 0 && (!HET || (d_off & 1) == 0), dx0 + 1 < dw);
    }
}

// Upsampling as a row walk: a lane owns 2 adjacent destination columns (one 16-B store per row, so that a store
// instruction of the wave writes 1 KiB contiguous) and walks down a segment of destination rows.  The (at most 3)
// source columns its pixels sample are loaded once per SOURCE row, blended horizontally once, and reused by the
// 2-3 destination rows that sample that source row.  Per-pixel arithmetic and its order are those of
// k_flow_upsample.
constexpr int UPW_SEG = 32;
template <bool FMA>
__global__ __launch_bounds__(256) void k_flow_upsample_walk(const float* __restrict__ src, int sw, int sh,
                                                             float* __restrict__ dst, int dw, int dh, double scale_x,
                                                             double scale_y, float mul)
{
    constexpr int NPL = 2, NV = NPL + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the 4 waves of a block take adjacent column chunks of the SAME rows: 4 KiB contiguous per row and block
    const int dx0 = ((blockIdx.x * 4 + wave) * 64 + lane) * NPL;
    const int y0 = blockIdx.y * UPW_SEG;
    if (y0 >= dh || (blockIdx.x * 4 + wave) * 64 * NPL >= dw) return;   // wave-uniform
    const int y1 = min(y0 + UPW_SEG, dh);
    const bool live = dx0 < dw;
    LinTap tx[NPL];   // indices relative to the first pixel's first column: i0 in 0..NPL-1, i1 in 0..NPL when upsampling
    int base = 0;
#pragma unroll
    for (int i = 0; i < NPL; i++) {
        tx[i] = lin_tap_x(min(dx0 + i, dw - 1), scale_x, sw);
        if (i == 0) base = tx[i].i0;
        tx[i].i0 -= base;
        tx[i].i1 -= base;
    }
    const float2* S = reinterpret_cast<const float2*>(src) + (size_t)blockIdx.z * sw * sh;
    float2* D = reinterpret_cast<float2*>(dst) + (size_t)blockIdx.z * dw * dh;
    auto pick = [](const float2 (&V)[NV], int k) {
        float2 r = V[0];
#pragma unroll
        for (int q = 1; q < NV; q++) r = k == q ? V[q] : r;
        return r;
    };
    // horizontal blend of source row r at the lane's destination columns
    auto hrow = [&](int r, float2 (&h)[NPL]) {
        const float2* row = S + (size_t)r * sw;
        float2 V[NV];
#pragma unroll
        for (int k = 0; k < NV; k++) V[k] = row[min(base + k, sw - 1)];
#pragma unroll
        for (int i = 0; i < NPL; i++) h[i] = lin_mix<FMA>(pick(V, tx[i].i0), pick(V, tx[i].i1), tx[i].w1);
    };
    float2 hA[NPL], hB[NPL];
    int ra = -1, rb = -1;
    for (int dy = y0; dy < y1; dy++) {
        const LinTap ty = lin_tap_y(dy, scale_y, sh);
        if (ty.i0 != ra) {                                    // all branches are wave-uniform
            if (ty.i0 == rb) {
#pragma unroll
                for (int i = 0; i < NPL; i++) hA[i] = hB[i];
            } else {
                hrow(ty.i0, hA);
            }
            ra = ty.i0;
        }
        const bool same = ty.i1 == ra;
        if (!same && ty.i1 != rb) {
            hrow(ty.i1, hB);
            rb = ty.i1;
        }
        if (live) {
            float2 o[NPL];
#pragma unroll
            for (int i = 0; i < NPL; i++) {
                const float2 t = lin_mix<FMA>(hA[i], same ? hA[i] : hB[i], ty.w1);
                o[i] = make_float2(t.x * mul, t.y * mul);
            }
            store_flow_pair(D + (size_t)dy * dw + dx0, o, dx0 + 1 < dw && (dw & 1) == 0, dx0 + 1 < dw);
        }
    }
}

}  // namespace

int nsof_launch_flow_upsample(nsof_ctx* ctx, int n_pairs, const float* src, int sw, int sh, float* dst, int dw, int dh, float mul)
{
    nsof_prof_scope ps(ctx, NSOF_K_UPSAMPLE);
    const double scale_x = inv_scale(dw, sw), scale_y = inv_scale(dh, sh);
    // upsampling: source steps of 0 or 1 between neighbours
    const bool up = dw >= sw && dh >= sh && sw >= 1 && sh >= 1;
    nsof_with_fma(ctx, [&](auto fma) {
        constexpr bool FMA = decltype(fma)::value;
        if (up && dw >= 256)   // rows wide enough for a lane per 2 columns
            hipLaunchKernelGGL(k_flow_upsample_walk<FMA>, dim3(((dw + 1) / 2 + 255) / 256, (dh + UPW_SEG - 1) / UPW_SEG, n_pairs),
                               dim3(256), 0, ctx->stream, src, sw, sh, dst, dw, dh, scale_x, scale_y, mul);
        else if (up)
            hipLaunchKernelGGL((k_flow_upsample2x2<false, FMA>), nsof_pixel_grid((dw + 1) / 2, (dh + 1) / 2, n_pairs), dim3(256),
                               0, ctx->stream, src, sw, sh, dst, dw, dh, scale_x, scale_y, mul, nullptr);
        else
            hipLaunchKernelGGL(k_flow_upsample<FMA>, nsof_pixel_grid(dw, dh, n_pairs), dim3(256), 0, ctx->stream, src, sw, sh,
                               dst, dw, dh, scale_x, scale_y, mul);
    });
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// Work list: field z of the launch is item z of the device table (max_w x max_h: the largest destination).
int nsof_launch_flow_upsample_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, int max_h,
                                  const float* src, float* dst, float mul)
{
    nsof_prof_scope ps(ctx, NSOF_K_UPSAMPLE);
    nsof_with_fma(ctx, [&](auto fma) {
        hipLaunchKernelGGL((k_flow_upsample2x2<true, decltype(fma)::value>), nsof_pixel_grid((max_w + 1) / 2, (max_h + 1) / 2, n_items),
                           dim3(256), 0, ctx->stream, src, 0, 0, dst, 0, 0, 1., 1., mul, d_items);
    });
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
