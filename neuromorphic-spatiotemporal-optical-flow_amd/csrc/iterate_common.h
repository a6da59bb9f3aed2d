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

// Where a thread's flow_in comes from: a policy type of the strip walker (k_iterate_x).  fetch(r) only issues the loads of
// image row r at the thread's column -> Pend (consumed windows later); value(pend, r) is the flow of that pixel.
//   bind(field, pair, plane, W)   this pair's field (HET: `field` is the item's own already)
//   column(xc)                    the thread's image column
// FlowSrc: the level's own flow buffer, one 8-byte load per row, value() is the identity.
struct FlowSrc {
    typedef float2 Pend;
    const char* base;   // flow_in of this pair
    unsigned W, xc;
    template <bool HET>
    __device__ __forceinline__ void bind(const float* field, int pair, size_t plane, int w)
    {
        base = reinterpret_cast<const char*>(field) + (HET ? 0 : (size_t)pair * plane * 8);
        W = (unsigned)w;
    }
    __device__ __forceinline__ void column(int c) { xc = (unsigned)c; }
    __device__ __forceinline__ float2 fetch(int r) const
    {
        return *reinterpret_cast<const float2*>(base + ((unsigned)r * W + xc) * 8u);
    }
    __device__ __forceinline__ float2 value(const float2& p, int) const { return p; }
};

// FlowResample2x: the flow of the COARSER level, pw x ph with W == 2 * pw and H == 2 * ph, resampled on the fly: for fine
// pixel (x, y) exactly what k_flow_upsample (farneback_resample.hip) writes and FlowSrc then reads,
//     t0 = p00*a0 + p01*a1;  t1 = p10*a0 + p11*a1;  o = (t0*b0 + t1*b1) * mul        (every a*b + c two roundings),
// with the coordinates, weights and clamps of lin_coord_x / lin_coord_y at scale 0.5.  The column pair and a0, a1 belong to
// the thread (column()).  Rows: at scale 0.5 the coordinate of row 2k + p is f = k + (p + 0.5) * 0.5 - 0.5, exact in double
// and in float (k < 2^21), so lin_coord_y(2k + p) = (k + sy(p), b1(p)): the helper is evaluated for rows 0 and 1 once
// (bind()) and a row costs a shift, an add and two clamps -- scalar work where the row is wave-uniform.
// A weight of zero does not excuse its load (0 * NaN is NaN): the clamped pixel is loaded and multiplied as k_flow_upsample
// does.  Every address is clamped into this pair's coarse field.
// Two forms.  The plain one (fetch / value, the policy's interface): the four 8-byte loads of a fine row stay pending -- 8
// registers where FlowSrc has 2 -- and every blend is done per fine row.  Four such rows in flight do not fit the strip
// walker's 168 registers (45-69 spilled), so its full producer waves, whose two rows per window are wave-uniform and
// adjacent, take the pair form (fetch2 / value2): a window's rows (ra, rb) = (i, i + 1), both clamped to H - 1, sample
//     i odd:   ra and rb both the coarse rows (s, s + 1), s = sy(ra)               -> X = s, Y = s + 1
//     i even:  ra the rows (s, s + 1), rb the rows (s + 1, s + 2)                  -> X = s + 1, Y = sy(rb) + 1
// (each clamped to the field), so a window loads the two rows X and Y at the thread's column pair (8 registers pending),
// blends each horizontally ONCE and uses it for both fine rows; for even i row s is the previous window's Y, whose blend
// is carried in two registers (z).  That holds with the clamps: H is even, so a clamped fine row is H - 1, odd, with
// sy = ph - 1, and clamp(ph) = clamp(ph - 1) = ph - 1; consecutive windows are i and i + 4.  The blends themselves are
// the expressions above on the same operands, shared as k_flow_upsample_walk shares them.
struct FlowResample2x {
    struct Pend {
        float2 p00, p01, p10, p11;
    };
    struct Pend2 {
        float2 x0, x1, y0, y1;   // coarse rows X and Y at the column pair
    };
    const char* base;   // coarse flow of this pair
    unsigned pw;
    int ph;
    float mul;
    int sy0, sy1;       // lin_coord_y of rows 0 and 1
    float b10, b11;
    unsigned c0, c1;    // byte offsets of the column pair in a coarse row
    float a0, a1;
    template <bool HET>
    __device__ __forceinline__ void bind(const float* field, int pair, size_t, int)
    {
        static_assert(!HET, "uniform batches only");
        base = reinterpret_cast<const char*>(field) + (size_t)pair * pw * (size_t)ph * 8;
        lin_coord_y(0, 0.5, sy0, b10);
        lin_coord_y(1, 0.5, sy1, b11);
        // wave-uniform by construction; say so, so that the per-row arithmetic stays on the scalar unit
        sy0 = __builtin_amdgcn_readfirstlane(sy0);
        sy1 = __builtin_amdgcn_readfirstlane(sy1);
        b10 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, b10)));
        b11 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, b11)));
    }
    __device__ __forceinline__ void column(int c)
    {
        int sx;
        lin_coord_x(c, 0.5, (int)pw, sx, a1);
        a0 = 1.f - a1;
        c0 = (unsigned)sx * 8u;
        c1 = (unsigned)min(sx + 1, (int)pw - 1) * 8u;
    }
    // lin_coord_y of fine row r: its upper coarse row (unclamped), and its weight b1
    __device__ __forceinline__ int row_sy(int r) const { return (r >> 1) + ((r & 1) ? sy1 : sy0); }
    __device__ __forceinline__ float row_b1(int r) const { return (r & 1) ? b11 : b10; }
    // byte offset of coarse row cr, clamped into the field
    __device__ __forceinline__ unsigned row_off(int cr) const { return (unsigned)clampi(cr, 0, ph - 1) * pw * 8u; }
    __device__ __forceinline__ float2 at(unsigned off) const { return *reinterpret_cast<const float2*>(base + off); }
    // t = p0*a0 + p1*a1 of one coarse row; o = (t0*b0 + t1*b1) * mul of fine row r
    __device__ __forceinline__ float2 hblend(const float2& p0, const float2& p1) const
    {
        return make_float2(nsof_madd<false>(p0.x, a0, p1.x * a1), nsof_madd<false>(p0.y, a0, p1.y * a1));
    }
    __device__ __forceinline__ float2 vblend(const float2& t0, const float2& t1, int r) const
    {
        const float b1 = row_b1(r), b0 = 1.f - b1;
        return make_float2(nsof_madd<false>(t0.x, b0, t1.x * b1) * mul, nsof_madd<false>(t0.y, b0, t1.y * b1) * mul);
    }
    // ---- the plain form
    __device__ __forceinline__ Pend fetch(int r) const
    {
        const int sy = row_sy(r);
        const unsigned r0 = row_off(sy), r1 = row_off(sy + 1);
        Pend p;
        p.p00 = at(r0 + c0);
        p.p01 = at(r0 + c1);
        p.p10 = at(r1 + c0);
        p.p11 = at(r1 + c1);
        return p;
    }
    __device__ __forceinline__ float2 value(const Pend& p, int r) const
    {
        return vblend(hblend(p.p00, p.p01), hblend(p.p10, p.p11), r);
    }
    // ---- the pair form: rows (ra, rb) of a window whose first stream index has parity ODD
    template <bool ODD>
    __device__ __forceinline__ Pend2 fetch2(int ra, int rb) const
    {
        const unsigned rx = row_off(row_sy(ra) + (ODD ? 0 : 1)), ry = row_off((ODD ? row_sy(ra) : row_sy(rb)) + 1);
        Pend2 q;
        q.x0 = at(rx + c0);
        q.x1 = at(rx + c1);
        q.y0 = at(ry + c0);
        q.y1 = at(ry + c1);
        return q;
    }
    // z: the blend of the previous window's row Y (ODD: unused)
    template <bool ODD>
    __device__ __forceinline__ void value2(const Pend2& q, float2& z, int ra, int rb, float2& oa, float2& ob) const
    {
        const float2 hx = hblend(q.x0, q.x1), hy = hblend(q.y0, q.y1);
        oa = ODD ? vblend(hx, hy, ra) : vblend(z, hx, ra);
        ob = vblend(hx, hy, rb);
        z = hy;
    }
    // the blend of the upper coarse row of fine row r, at once: the first even window's z
    __device__ __forceinline__ float2 upper_row(int r) const
    {
        const unsigned r0 = row_off(row_sy(r));
        return hblend(at(r0 + c0), at(r0 + c1));
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
