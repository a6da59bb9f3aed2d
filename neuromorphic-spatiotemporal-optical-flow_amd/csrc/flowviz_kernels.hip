// Middlebury colour coding of flow fields on the device (flow_viz.flow_to_image; optical_flow_prediction.py:12-19,
// :524, :578): the script's `viz` of the gated and the full-frame flow of every pair, without the 8 B/px float32 flow
// crossing PCIe or the 0.2 s per 1080p flow of the NumPy mirror (nsof/flowviz.py).
//
//   k_flowviz_max     largest magnitude sqrt(u*u + v*v) of each item (float32, no FMA): wave max, workgroup max
//                     through LDS, one atomicMax per workgroup on the bit pattern of the non-negative float in the
//                     item's slot.  A max does not depend on order, so the slot is bit-reproducible.
//   k_flowviz_color   per pixel: u/d, v/d (d = max + 1e-5 in float32, or the caller's float32(max_flow + 1e-5)), the
//                     wheel position in float32 from a float64 atan2 rounded once to float32, the blend and the
//                     saturation in float64, floor(255 * col) to uint8.
//
// Numerics are those of nsof.flow_to_image on float32 input under NumPy 2 promotion (NEP 50): every float32 step
// rounds as NumPy rounds it (-ffp-contract=off, __f*_rn, sqrtf), frac = pos - lo is float64 because float32 minus int32
// promotes, and atan2 is defined as (float)atan2((double)y, (double)x) -- NumPy's own float32 arctan2 is not
// correctly rounded and depends on the host's SIMD dispatch.  Signed zeros are kept as NumPy keeps them: the sign
// flip and the negations inside atan2 are sign-bit flips, np.clip(x, 0, c) keeps -0.0 (only x < 0 becomes +0.0), and
// the division keeps the sign of a zero, so atan2(+-0, negative) lands on wheel entry 54 or 0 as on the host.
//
// Non-finite flows, where the NumPy coding has no answer (np.max propagates a NaN into every pixel's divisor, and a NaN
// wheel position cannot index the wheel), are defined here instead:
//   * the divisor is the largest magnitude over the pixels whose magnitude is not NaN (fmaxf skips NaN), + 1e-5;
//     an infinite component makes it +inf, and every finite component then codes as 0 -- unless the pixel's other
//     component is NaN: sqrt(inf + NaN) is NaN, so (inf, NaN) is skipped like any NaN pixel.  A finite component whose
//     square overflows float32 (3e38) has the magnitude +inf too;
//   * a pixel whose normalised u or v is NaN (a NaN flow, or an infinite one over an infinite divisor) is (0, 0, 0),
//     a colour no finite flow produces: one wheel channel is always 255 inside the unit circle and 191 outside;
//   * an infinite normalised component (a finite divisor from max_flow) is an ordinary pixel outside the unit circle:
//     atan2 of infinities is finite, so it gets the wheel colour of its direction times 0.75, as in NumPy.
// Thread layout of both kernels: a wave covers 256 consecutive pixels of a row (4 per lane), a workgroup 4 waves, each
// wave RPW rows; blockIdx.z = item.  V4: every row starts 16-byte aligned, so a lane's 4 pixels are two float4 loads.
#include <cmath>

#include "nsof_internal.h"

namespace {

constexpr int PX = 4;                  // pixels per lane
constexpr int RPW = 4;                 // rows per wave
constexpr int BX = 64 * PX;            // pixels per workgroup along x
constexpr int BY = 4 * RPW;            // rows per workgroup
constexpr int NCOLS = 55;              // make_colorwheel(): RY 15, YG 6, GC 4, CB 11, BM 13, MR 6
constexpr float PI_F = 3.14159265358979323846f;   // float32(np.pi), as NumPy 2 divides a float32 array by np.pi

struct Wheel {
    double v[NCOLS][3];
};

// make_colorwheel() / 255.0: each segment holds one channel at 255 and ramps another by floor(255 * i / k) (an integer
// quotient here; the float64 quotient of the host cannot round across an integer), up or down.
constexpr Wheel make_wheel()
{
    Wheel w{};
    const int seg[6] = {15, 6, 4, 11, 13, 6};
    const int hold[6] = {0, 1, 1, 2, 2, 0}, ramp[6] = {1, 0, 2, 1, 0, 2}, up[6] = {1, 0, 1, 0, 1, 0};
    int at = 0;
    for (int s = 0; s < 6; s++)
        for (int i = 0; i < seg[s]; i++, at++) {
            const int step = 255 * i / seg[s];
            w.v[at][hold[s]] = 255 / 255.0;
            w.v[at][ramp[s]] = (up[s] ? step : 255 - step) / 255.0;
        }
    return w;
}

__constant__ Wheel c_wheel = make_wheel();

// flow := sign * flow, then np.clip(flow, 0, clip) when CLIP: x < 0 -> +0.0 (-0.0 stays), x > clip -> clip.
template <bool CLIP>
__device__ __forceinline__ float prep(float f, bool neg, float clip)
{
    if (neg) f = -f;
    if (CLIP) {
        if (f < 0.f) f = 0.f;
        if (f > clip) f = clip;
    }
    return f;
}

// np.sqrt(np.square(u) + np.square(v)) in float32.  sqrtf, not __fsqrt_rn: HIP maps __fsqrt_rn to the native v_sqrt_f32
// (about 1 ulp) unless OCML_BASIC_ROUNDED_OPERATIONS is defined, while sqrtf is correctly rounded (hipcc's default
// -fhip-fp32-correctly-rounded-divide-sqrt), as NumPy's is.  sqrt(1 - 2^-24) is one case that tells them apart.
__device__ __forceinline__ float mag(float u, float v)
{
    return sqrtf(__fadd_rn(__fmul_rn(u, u), __fmul_rn(v, v)));
}

// The (u, v) of pixels x0 .. x0+3 of row `r` (pixels at or past w are not read; their values are 0).
template <bool V4>
__device__ __forceinline__ void load4(const float* __restrict__ r, int x0, int w, float (&f)[2 * PX])
{
    if (V4 && x0 + PX <= w) {
        const float4 a = *reinterpret_cast<const float4*>(r + 2 * x0);
        const float4 b = *reinterpret_cast<const float4*>(r + 2 * x0 + 4);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
        f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
#pragma unroll
        for (int j = 0; j < PX; j++) {
            const bool in = x0 + j < w;
            f[2 * j] = in ? r[2 * (x0 + j)] : 0.f;
            f[2 * j + 1] = in ? r[2 * (x0 + j) + 1] : 0.f;
        }
    }
}

template <bool V4, bool CLIP>
__global__ __launch_bounds__(256) void k_flowviz_max(const float* __restrict__ flows, ptrdiff_t rs, ptrdiff_t is, int w,
                                                     int h, int neg, float clip, unsigned* __restrict__ slots)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, z = blockIdx.z;
    const int x0 = (blockIdx.x * 64 + lane) * PX;
    const float* item = flows + (ptrdiff_t)z * is;
    float m = 0.f;
    if (x0 < w) {
#pragma unroll
        for (int r = 0; r < RPW; r++) {
            const int y = blockIdx.y * BY + r * 4 + wave;
            if (y >= h) break;
            float f[2 * PX];
            load4<V4>(item + (ptrdiff_t)y * rs, x0, w, f);
#pragma unroll
            for (int j = 0; j < PX; j++)   // pixels past w read as (0, 0): magnitude 0 never raises the max
                m = fmaxf(m, mag(prep<CLIP>(f[2 * j], neg, clip), prep<CLIP>(f[2 * j + 1], neg, clip)));
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    __shared__ float part[4];
    if (lane == 0) part[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        atomicMax(slots + z, __float_as_uint(m));   // m >= +0: the uint order of the bits is the float order
    }
}

// One pixel's three channels, in the order the host writes them: col = (1 - frac) * wheel[lo] + frac * wheel[hi],
// then 1 - rad * (1 - col) inside the unit circle or col * 0.75 outside, then floor(255 * col).
__device__ __forceinline__ void color_px(float u, float v, uint8_t (&o)[3])
{
    if (u != u || v != v) {   // NaN: no wheel position (see the header); black marks the pixel
        o[0] = o[1] = o[2] = 0;
        return;
    }
    const float rad = mag(u, v);
    const float a = (float)atan2(-(double)v, -(double)u);
    const float pos = __fmul_rn(__fdiv_rn(__fadd_rn(__fdiv_rn(a, PI_F), 1.f), 2.f), (float)(NCOLS - 1));
    int lo = (int)floorf(pos);
    lo = min(max(lo, 0), NCOLS - 1);   // pos is in [0, 54] for non-NaN input; the clamp keeps any index in the table
    const int hi = lo + 1 == NCOLS ? 0 : lo + 1;
    const double frac = (double)pos - (double)lo;
    const bool small = rad <= 1.f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double col = (1.0 - frac) * c_wheel.v[lo][c] + frac * c_wheel.v[hi][c];
        col = small ? 1.0 - (double)rad * (1.0 - col) : col * 0.75;
        o[c] = (uint8_t)floor(255.0 * col);
    }
}

// GIVEN: the divisor is the caller's; else slots[z] holds the item's max magnitude bits.  The first workgroup of each
// item writes the divisor to norms[z] when norms is given.
template <bool V4, bool CLIP, bool GIVEN>
__global__ __launch_bounds__(256) void k_flowviz_color(const float* __restrict__ flows, ptrdiff_t rs, ptrdiff_t is,
                                                       int w, int h, int neg, float clip,
                                                       const unsigned* __restrict__ slots, float given, int bgr,
                                                       uint8_t* __restrict__ out, ptrdiff_t ors, ptrdiff_t ois,
                                                       float* __restrict__ norms)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, z = blockIdx.z;
    const float d = GIVEN ? given : __fadd_rn(__uint_as_float(slots[z]), 1e-5f);
    if (norms && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) norms[z] = d;
    const int x0 = (blockIdx.x * 64 + lane) * PX;
    if (x0 >= w) return;
    const float* item = flows + (ptrdiff_t)z * is;
    uint8_t* oitem = out + (ptrdiff_t)z * ois;
    const int c0 = bgr ? 2 : 0, c2 = bgr ? 0 : 2;
#pragma unroll 1
    for (int r = 0; r < RPW; r++) {
        const int y = blockIdx.y * BY + r * 4 + wave;
        if (y >= h) break;
        float f[2 * PX];
        load4<V4>(item + (ptrdiff_t)y * rs, x0, w, f);
        uint8_t px[PX * 3];
#pragma unroll
        for (int j = 0; j < PX; j++) {
            uint8_t o[3];
            color_px(__fdiv_rn(prep<CLIP>(f[2 * j], neg, clip), d), __fdiv_rn(prep<CLIP>(f[2 * j + 1], neg, clip), d), o);
            px[3 * j + c0] = o[0];
            px[3 * j + 1] = o[1];
            px[3 * j + c2] = o[2];
        }
        uint8_t* o = oitem + (ptrdiff_t)y * ors + 3 * x0;
        if (x0 + PX <= w && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            unsigned* o32 = reinterpret_cast<unsigned*>(o);
#pragma unroll
            for (int k = 0; k < 3; k++)
                o32[k] = px[4 * k] | px[4 * k + 1] << 8 | px[4 * k + 2] << 16 | (unsigned)px[4 * k + 3] << 24;
        } else {
            for (int k = 0; k < 3 * min(PX, w - x0); k++) o[k] = px[k];
        }
    }
}

template <bool V4, bool CLIP>
void launch_color(nsof_ctx* ctx, dim3 grid, bool given, const float* flows, ptrdiff_t rs, ptrdiff_t is, int w, int h,
                  int neg, float clip, const unsigned* slots, float div, int bgr, uint8_t* out, ptrdiff_t ors,
                  ptrdiff_t ois, float* norms)
{
    if (given)
        hipLaunchKernelGGL((k_flowviz_color<V4, CLIP, true>), grid, dim3(256), 0, ctx->stream, flows, rs, is, w, h, neg,
                           clip, slots, div, bgr, out, ors, ois, norms);
    else
        hipLaunchKernelGGL((k_flowviz_color<V4, CLIP, false>), grid, dim3(256), 0, ctx->stream, flows, rs, is, w, h,
                           neg, clip, slots, div, bgr, out, ors, ois, norms);
}

template <bool V4, bool CLIP>
void launch_both(nsof_ctx* ctx, dim3 grid, bool given, const float* flows, ptrdiff_t rs, ptrdiff_t is, int w, int h,
                 int neg, float clip, unsigned* slots, float div, int bgr, uint8_t* out, ptrdiff_t ors, ptrdiff_t ois,
                 float* norms)
{
    if (!given)
        hipLaunchKernelGGL((k_flowviz_max<V4, CLIP>), grid, dim3(256), 0, ctx->stream, flows, rs, is, w, h, neg, clip,
                           slots);
    launch_color<V4, CLIP>(ctx, grid, given, flows, rs, is, w, h, neg, clip, slots, div, bgr, out, ors, ois, norms);
}

}  // namespace

extern "C" int nsof_flow_to_image_dev(nsof_ctx* ctx, int n, const float* d_flows, ptrdiff_t row_stride_floats,
                                      ptrdiff_t item_stride_floats, int width, int height, int sign, double clip_flow,
                                      double max_flow, int convert_to_bgr, uint8_t* d_out, ptrdiff_t out_row_stride,
                                      ptrdiff_t out_item_stride, float* d_norms)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_flows || !d_out) return nsof_set_error(ctx, NSOF_EINVAL, "flow_to_image: null pointer");
    if (n <= 0 || width <= 0 || height <= 0)
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_to_image: n %d, size %dx%d", n, width, height);
    if (row_stride_floats < 2 * (ptrdiff_t)width || out_row_stride < 3 * (ptrdiff_t)width)
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_to_image: row stride shorter than a row");
    // items must not overlap: each item's stride at least its footprint (first byte of row 0 .. last byte of row h-1)
    if (n > 1 && (item_stride_floats < (ptrdiff_t)(height - 1) * row_stride_floats + 2 * (ptrdiff_t)width ||
                  out_item_stride < (ptrdiff_t)(height - 1) * out_row_stride + 3 * (ptrdiff_t)width))
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_to_image: item strides make items overlap");
    if (sign != 1 && sign != -1) return nsof_set_error(ctx, NSOF_EINVAL, "flow_to_image: sign must be +1 or -1");
    if (!(clip_flow == clip_flow) || !(max_flow == max_flow))
        return nsof_set_error(ctx, NSOF_EINVAL, "flow_to_image: NaN clip_flow / max_flow");
    if (n > 65535) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "flow_to_image: more than 65535 items");
    const dim3 grid((width + BX - 1) / BX, (height + BY - 1) / BY, n);
    if (grid.y > 65535) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "flow_to_image: height %d", height);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const bool given = max_flow >= 0, clip = clip_flow >= 0;
    const float div = given ? (float)(max_flow + 1e-5) : 0.f, c = clip ? (float)clip_flow : 0.f;
    const int neg = sign < 0;
    unsigned* slots = nullptr;
    if (!given) {
        int rc = ctx->tmp.reserve(ctx, (size_t)n * sizeof(unsigned));
        if (rc) return rc;
        slots = (unsigned*)ctx->tmp.p;
        NSOF_HIP(ctx, hipMemsetAsync(slots, 0, (size_t)n * sizeof(unsigned), ctx->stream));
    }
    const bool v4 = (reinterpret_cast<uintptr_t>(d_flows) & 15) == 0 && row_stride_floats % 4 == 0 &&
                    (n == 1 || item_stride_floats % 4 == 0);
    if (v4 && clip)
        launch_both<true, true>(ctx, grid, given, d_flows, row_stride_floats, item_stride_floats, width, height, neg, c,
                                slots, div, convert_to_bgr, d_out, out_row_stride, out_item_stride, d_norms);
    else if (v4)
        launch_both<true, false>(ctx, grid, given, d_flows, row_stride_floats, item_stride_floats, width, height, neg, c,
                                 slots, div, convert_to_bgr, d_out, out_row_stride, out_item_stride, d_norms);
    else if (clip)
        launch_both<false, true>(ctx, grid, given, d_flows, row_stride_floats, item_stride_floats, width, height, neg, c,
                                 slots, div, convert_to_bgr, d_out, out_row_stride, out_item_stride, d_norms);
    else
        launch_both<false, false>(ctx, grid, given, d_flows, row_stride_floats, item_stride_floats, width, height, neg,
                                  c, slots, div, convert_to_bgr, d_out, out_row_stride, out_item_stride, d_norms);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
