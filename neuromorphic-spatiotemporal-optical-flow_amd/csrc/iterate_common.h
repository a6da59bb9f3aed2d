// Device helpers shared by the Farneback iteration kernels (farneback_iterate*.hip):
// the expansion layout, the per-row load bundle of a pixel, FarnebackUpdateMatrices for one pixel, the flow source.
#pragma once
#include <atomic>
#include <cstdlib>
#include <type_traits>

#include "nsof_internal.h"

namespace {

// R of one image: [h][w][4] f32 (channels 0-3 of a pixel = one aligned 16-B access) followed by [h][w] f32
// (channel 4).  32-bit byte offsets against wave-uniform bases keep every load in the "SGPR base + VGPR offset"
// form.  The L1 serves 4 lanes per cycle whatever the access width, so a thread-row costs 9 loads here
// (R0: x4 + x1; R1: 2 rows x (x4, x4, x2)) instead of 15 with planar channels.
struct Planes {
    const char* q4;   // interleaved channels 0..3
    const char* c4;   // channel 4
};
struct __attribute__((packed, aligned(4))) f2u {  // two adjacent floats, only 4-byte aligned
    float a, b;
};
__device__ __forceinline__ Planes planes_of(const float* img_base, size_t plane)
{
    Planes p;
    p.q4 = reinterpret_cast<const char*>(img_base);
    p.c4 = reinterpret_cast<const char*>(img_base + 4 * plane);
    return p;
}

struct RowIn {
    float4 z;             // R0 channels 0..3
    float z4;             // R0 channel 4
    float4 t0, t1, b0, b1;  // R1 channels 0..3 at (y1,x1), (y1,x1+1), (y1+1,x1), (y1+1,x1+1)
    f2u t4, b4;           // R1 channel 4 at (y1, x1..x1+1) and (y1+1, x1..x1+1)
    float fx, fy;
    int inside;
};

// Issue every load one (row, column) needs; `d` is the flow at that pixel (already loaded; matrix_from takes it again).
// W >= 2 and H >= 2 (nsof_iterate_supported): the clamped gather needs a 2x2 block.
//
// Sample coordinates without a branch: flx = floorf(fx) (v_floor_f32), the fraction fx - flx, `inside` decided on flx in
// float, and an integer only for the clamped gather address.  This gives the M of the form it replaces
// (x1 = floor_f(fx), fraction fx - x1, inside = 0 <= x1 <= W-2), bit for bit:
//   * |fx| < 2^31: floorf(fx) == (float)floor_f(fx) exactly (below 2^24 both are the same small integer; from 2^24 on fx is
//     an integer itself and floor_f(fx) a multiple of the float spacing there), so the fraction is the same operation on
//     the same operands, and flx >= 0 && flx <= W-2 is x1 >= 0 && x1 <= W-2 (W-2 < 2^24 is exact as a float);
//   * NaN, +-inf, |fx| >= 2^31: floor_f gives INT_MIN / INT_MAX, outside; here NaN fails both comparisons and the others
//     fail one of them: outside in both forms;
//   * outside, only the clamped address uses the index, and matrix_from does not read what that load returns (nor the
//     fraction, which may be NaN here);
//   * fx = x + d.x with x >= 0 from an integer is never -0.0 (x + d.x == 0 rounds to +0 for x > 0, and for x == 0 a d.x
//     of -0.0 gives 0 + -0 = +0), so neither floorf nor the subtraction sees a signed zero the integer form did not.
__device__ __forceinline__ void issue_row(RowIn& in, const Planes& R0, const Planes& R1, int W, int H, int x, int y,
                                          float2 d)
{
    const unsigned pix = (unsigned)y * (unsigned)W + (unsigned)x;
    const float fx = x + d.x, fy = y + d.y;
    const float flx = __builtin_floorf(fx), fly = __builtin_floorf(fy);
    const float xhi = (float)(W - 2), yhi = (float)(H - 2);
    in.fx = fx - flx;
    in.fy = fy - fly;
    in.inside = flx >= 0.f && flx <= xhi && fly >= 0.f && fly <= yhi;
    in.z = *reinterpret_cast<const float4*>(R0.q4 + pix * 16u);
    in.z4 = *reinterpret_cast<const float*>(R0.c4 + pix * 4u);
    // The R1 gather is issued unconditionally, at a clamped (always valid) address when the sample falls
    // outside: a load under a lane-dependent branch cannot be counted by s_waitcnt vmcnt(N), which would
    // force every wait down to "almost nothing outstanding" and serialise the software pipeline.
    // Clamped in float, one v_med3_f32 each (0 <= hi: see above; a NaN gives the lower bound), then converted.
    const int xs = (int)__builtin_amdgcn_fmed3f(flx, 0.f, xhi), ys = (int)__builtin_amdgcn_fmed3f(fly, 0.f, yhi);
    const unsigned o = (unsigned)ys * (unsigned)W + (unsigned)xs;
    in.t0 = *reinterpret_cast<const float4*>(R1.q4 + o * 16u);
    in.t1 = *reinterpret_cast<const float4*>(R1.q4 + o * 16u + 16u);
    in.b0 = *reinterpret_cast<const float4*>(R1.q4 + (o + (unsigned)W) * 16u);
    in.b1 = *reinterpret_cast<const float4*>(R1.q4 + (o + (unsigned)W) * 16u + 16u);
    in.t4 = *reinterpret_cast<const f2u*>(R1.c4 + o * 4u);
    in.b4 = *reinterpret_cast<const f2u*>(R1.c4 + (o + (unsigned)W) * 4u);
}

// FarnebackUpdateMatrices for one pixel, from loaded inputs and the flow (dx, dy) issue_row was given for it.
__device__ __forceinline__ void matrix_from(const RowIn& in, float dx, float dy, int x, int y, int W, int H, float (&M)[5])
{
    float r2, r3, r4, r5, r6;
    if (in.inside) {
        const float fx = in.fx, fy = in.fy;
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        r2 = a00 * in.t0.x + a01 * in.t1.x + a10 * in.b0.x + a11 * in.b1.x;
        r3 = a00 * in.t0.y + a01 * in.t1.y + a10 * in.b0.y + a11 * in.b1.y;
        r4 = a00 * in.t0.z + a01 * in.t1.z + a10 * in.b0.z + a11 * in.b1.z;
        r5 = a00 * in.t0.w + a01 * in.t1.w + a10 * in.b0.w + a11 * in.b1.w;
        r6 = a00 * in.t4.a + a01 * in.t4.b + a10 * in.b4.a + a11 * in.b4.b;
        r4 = (in.z.z + r4) * 0.5f;
        r5 = (in.z.w + r5) * 0.5f;
        r6 = (in.z4 + r6) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = in.z.z;
        r5 = in.z.w;
        r6 = in.z4 * 0.5f;
    }
    r2 = (in.z.x - r2) * 0.5f;
    r3 = (in.z.y - r3) * 0.5f;
    r2 += r4 * dy + r6 * dx;
    r3 += r6 * dy + r5 * dx;
    if ((unsigned)(x - 5) >= (unsigned)(W - 10) || (unsigned)(y - 5) >= (unsigned)(H - 10)) {
        auto bw = [](int i) { return i < 2 ? 0.14f : 0.4472f; };
        const float scale = (x < 5 ? bw(x) : 1.f) * (x >= W - 5 ? bw(W - x - 1) : 1.f) * (y < 5 ? bw(y) : 1.f) *
                            (y >= H - 5 ? bw(H - y - 1) : 1.f);
        r2 *= scale; r3 *= scale; r4 *= scale; r5 *= scale; r6 *= scale;
    }
    M[0] = r4 * r4 + r6 * r6;
    M[1] = (r4 + r5) * r6;
    M[2] = r5 * r5 + r6 * r6;
    M[3] = r4 * r2 + r6 * r3;
    M[4] = r6 * r2 + r5 * r3;
}

// Where a thread's flow_in comes from: the level's own flow buffer.  fetch() only issues the load (the result is
// consumed windows later).
struct FlowSrc {
    const char* base;   // flow_in of this pair
    unsigned W, xc;
    __device__ __forceinline__ float2 fetch(int r) const
    {
        return *reinterpret_cast<const float2*>(base + ((unsigned)r * W + xc) * 8u);
    }
};

// > 64 KB of dynamic LDS needs the opt-in attribute, once per (kernel instance, device); contexts of several
// devices and the worker threads of a stream pool may arrive here concurrently.
template <typename K>
int lds_opt_in(nsof_ctx* ctx, K kernel, size_t bytes)
{
    static std::atomic<unsigned long long> done{0};   // one bit per device ordinal (per template instance)
    const unsigned long long bit = 1ull << (ctx->device & 63);
    if (done.load(std::memory_order_acquire) & bit) return NSOF_OK;
    NSOF_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done.fetch_or(bit, std::memory_order_release);
    return NSOF_OK;
}

}  // namespace
