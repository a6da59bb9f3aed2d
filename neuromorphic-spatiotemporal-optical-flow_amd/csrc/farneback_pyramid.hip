// Farneback dense optical flow, pyramid stage: the pyramid-level kernels (k_prep_*) for gfx950 (CDNA4, wave64).  The
// coarse-to-fine flow resample is in farneback_resample.hip, the expansion in farneback_polyexp.hip, the unfused
// box-window solve in farneback_blur.hip, the iterations in farneback_iterate*.hip.
//
// Layout of this file: pixel access and the two filters; the shared pieces of the resampling kernels (window loads,
// the resample tail); the kernels, one per route; the launchers -- prep_route()
// names the route of a uniform level, prep_impl() launches it.
//
// Replaces the arithmetic the reference obtains from cv2.calcOpticalFlowFarneback
// (call sites: /root/reference/optical_flow_seg.py:158,203,494 and the ob/prediction/yolo
// twins).  Every kernel keeps the reference library's operation order and float/double
// placement (see DESIGN.md "numerics contract"); this translation unit is compiled with
// -ffp-contract=off so that a*b+c stays two roundings unless fma() is written explicitly.
//
// All kernels are HBM/L2-bound stencils: no MFMA.  Layouts: images [n][h][w] f32, flow [n][h][w][2].
//
// Every kernel and the helpers between them take the arithmetic variant as their last template argument FMA: each tap
// and blend is nsof_madd<FMA> (nsof_internal.h), the plain multiply-then-add or one fused multiply-add.  The launchers at
// the end of the file read the variant from ctx->opt_pyr_fma (NSOF_OPT_PYR_FMA).
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "nsof_internal.h"

namespace {

// (resize(INTER_LINEAR) taps and blends: lin_tap_x / lin_tap_y, lin_mix, lin_blend, nsof_internal.h)

// ---------------------------------------------------------------------------------------
// Pyramid level preparation: u8 / f32 -> f32, separable Gaussian (sepFilter2D order), bilinear
// resample of the blurred FULL-RES image to (wk, hk).
// ---------------------------------------------------------------------------------------

// Source frames are 8-bit (T = uint8_t), 16-bit (uint16_t, int16_t) or float (T = float); row and image strides are in
// BYTES for all.  px() is the one load-and-convert of a source pixel (integers: the exact conversion; f32: the value
// itself), srow() the start of a byte-strided row.  For T = uint8_t both are exactly the expressions the 8-bit kernels
// always had.
template <typename T>
__device__ __forceinline__ float px(const T* p) { return (float)*p; }
template <typename T>
__device__ __forceinline__ const T* srow(const T* img, ptrdiff_t r, ptrdiff_t stride)
{
    return reinterpret_cast<const T*>(reinterpret_cast<const char*>(img) + r * stride);
}
// Pixel-width trait.  Integer frames (8- and 16-bit) are read as packed dwords of kPPD<T> pixels where the kernels load
// raw bytes; px_el<T>(v, e) is the exact conversion of pixel e of such a dword (unsigned: zero-extended, int16_t:
// sign-extended) -- for uint8_t the expression the 8-bit kernels always had.
template <typename T>
constexpr bool kU8 = std::is_same<T, uint8_t>::value;
template <typename T>
constexpr bool kInt = std::is_integral<T>::value;
template <typename T>
constexpr int kPPD = kInt<T> ? 4 / (int)sizeof(T) : 1;
template <typename T>
__device__ __forceinline__ float px_el(unsigned v, int e)
{
    if constexpr (sizeof(T) == 1) return (float)((v >> (8 * e)) & 0xffu);
    else if constexpr (std::is_signed<T>::value) return (float)(int)(short)(v >> (16 * e));
    else return (float)((v >> (16 * e)) & 0xffffu);
}
// Four adjacent pixels of a row as one aligned vector (8-bit: a dword, 16-bit: 8 bytes, float: 16), and pixel e of it.
template <typename T>
using PxQuad = std::conditional_t<sizeof(T) == 1, unsigned, std::conditional_t<sizeof(T) == 2, uint2, float4>>;
template <typename T>
__device__ __forceinline__ float quad_el(const PxQuad<T>& v, int e)
{
    if constexpr (sizeof(T) == 1) return px_el<T>(v, e);
    else if constexpr (sizeof(T) == 2) return px_el<T>(e < 2 ? v.x : v.y, e & 1);
    else return e == 0 ? v.x : (e == 1 ? v.y : (e == 2 ? v.z : v.w));
}

// Row filter at an (unreflected) column c of one row, ordering per kernel size.
// KS > 0: kernel size known at compile time (loops unroll, taps are scalar registers); KS == 0: runtime size,
// the tap accessor `tk(j)` then reads a copy of the taps in LDS (a dynamically indexed kernel argument, or a
// pointer to it, would be one dependent memory load per tap -- measured 10x slower).
template <int KS, bool FMA, typename TapF, typename LoadF>
__device__ __forceinline__ float row_filter(TapF tk, int ksize, int c, LoadF ld)
{
    const int ks = KS ? KS : ksize, r = ks >> 1;
    if (ks == 3) return nsof_madd<FMA>(ld(c - 1) + ld(c + 1), tk(2), ld(c) * tk(1));
    if (ks == 5) return nsof_madd<FMA>(ld(c - 2) + ld(c + 2), tk(4), nsof_madd<FMA>(ld(c - 1) + ld(c + 1), tk(3), ld(c) * tk(2)));
    float s = tk(0) * ld(c - r);
#pragma unroll
    for (int j = 1; j < ks; j++) s = nsof_madd<FMA>(tk(j), ld(c - r + j), s);
    return s;
}
// Column filter at (unreflected) row rr given an accessor of row-filtered values.
template <int KS, bool FMA, typename TapF, typename LoadF>
__device__ __forceinline__ float col_filter(TapF tk, int ksize, int rr, LoadF hv)
{
    const int ks = KS ? KS : ksize, r = ks >> 1;
    if (ks == 3) return nsof_madd<FMA>(hv(rr - 1) + hv(rr + 1), tk(2), hv(rr) * tk(1));
    float s = tk(r) * hv(rr);
#pragma unroll
    for (int j = 1; j <= r; j++) s = nsof_madd<FMA>(tk(r + j), hv(rr + j) + hv(rr - j), s);
    return s;
}
// The run-time taps of a block in LDS (see row_filter): threads first .. first + NSOF_MAX_BLUR_TAPS - 1 copy one each;
// the caller's barrier publishes them.
__device__ __forceinline__ void stage_taps(float (&s_tk)[NSOF_MAX_BLUR_TAPS], const nsof_blur_taps& t, int first = 0)
{
    const int j = (int)threadIdx.x - first;
    if ((unsigned)j < (unsigned)NSOF_MAX_BLUR_TAPS) s_tk[j] = t.k[j];
}

// ---- the N pixels of a row from column c on, as floats ----------------------------------------------------------------
// Fast form, for a window that lies inside the row: integer frames as unaligned dword loads of kPPD<T> pixels each
// (the last one may reach up to kPPD<T> - 1 pixels past the window: window_fast() keeps that inside the row as well),
// float frames pixel by pixel.
template <typename T>
using WinWord = std::conditional_t<kInt<T>, unsigned, float>;
template <typename T, int N>
constexpr int kWinWords = (N + kPPD<T> - 1) / kPPD<T>;
template <typename T, int N, typename C>
__device__ __forceinline__ void load_window(const T* rowp, C c, float (&b)[N])
{
    WinWord<T> raw[kWinWords<T, N>];
#pragma unroll
    for (int d = 0; d < kWinWords<T, N>; d++) __builtin_memcpy(&raw[d], rowp + c + kPPD<T> * d, 4);
#pragma unroll
    for (int d = 0; d < kWinWords<T, N>; d++)
#pragma unroll
        for (int e = 0; e < kPPD<T>; e++)
            if (kPPD<T> * d + e < N) {
                if constexpr (kInt<T>) b[kPPD<T> * d + e] = px_el<T>(raw[d], e);
                else b[d] = raw[d];
            }
}
// Border form: pixel by pixel with BORDER_REFLECT_101 columns.
template <typename T, int N>
__device__ __forceinline__ void load_window_reflect(const T* rowp, int c, int W, float (&b)[N])
{
#pragma unroll
    for (int j = 0; j < N; j++) b[j] = px(rowp + reflect101(c + j, W));
}
// May the N-pixel window that starts R columns left of column c take the fast form?  With two columns: and is c1 the
// column after c0, so that one window of KS + 1 pixels serves the row filter at both?
template <typename T, int N>
__device__ __forceinline__ bool window_fast(int c, int R, int W)
{
    return c - R >= 0 && c - R + kPPD<T> * kWinWords<T, N> <= W;
}
template <typename T, int N>
__device__ __forceinline__ bool window_fast(int c0, int c1, int R, int W)
{
    return window_fast<T, N>(c0, R, W) && c1 == c0 + 1;
}

// ---- shared by the kernels that resample in registers (direct, cols) ---------------------------------------------------
// The resample tail.  hv0(q) / hv1(q): the row-filtered values at a destination pixel's two columns of source row
// r0 - R + q, q = 0 .. KS.  Column filter at r0 (window entry R), at r1 = r0 + 1 (entry R + 1) unless the two rows are
// one (`two_rows`: r1 != r0), then resize's 2x2 blend with the column weight a1 and the row weight b1.
template <int KS, bool FMA, typename TapF, typename H0F, typename H1F>
__device__ __forceinline__ float resample_tail(TapF tk, H0F hv0, H1F hv1, bool two_rows, float a1, float b1)
{
    constexpr int R = KS / 2;
    const float B00 = col_filter<KS, FMA>(tk, KS, R, hv0);
    const float B01 = col_filter<KS, FMA>(tk, KS, R, hv1);
    float B10 = B00, B11 = B01;
    if (two_rows) {
        B10 = col_filter<KS, FMA>(tk, KS, R + 1, hv0);
        B11 = col_filter<KS, FMA>(tk, KS, R + 1, hv1);
    }
    return lin_blend<FMA>(B00, B01, B10, B11, a1, b1);
}

// Geometry of one image of a pyramid-level launch.  HET == false: the uniform batch (every image has the kernel
// arguments' shape, image z lives at src + z*img_stride and goes to out + z*wk*hk).  HET == true: image z belongs to
// work item z/2 of the device table (z & 1: prev / next), see nsof_het_item.
template <typename T>
struct PrepImg {
    const T* img;
    float* dst;
};
template <bool HET, typename T>
__device__ __forceinline__ bool prep_geom(PrepImg<T>& g, const T* src, ptrdiff_t& row_stride, ptrdiff_t img_stride,
                                          int& W, int& H, int& wk, int& hk, float* out,
                                          const nsof_het_item* __restrict__ items, int want_flag)
{
    if constexpr (HET) {   // (a list's frames are all of one pixel type, the launch's T)
        const nsof_het_item& it = items[blockIdx.z >> 1];
        const int which = blockIdx.z & 1;
        if (want_flag >= 0 && (it.flags & NSOF_HET_VEC0) != want_flag) return false;
        W = it.W; H = it.H; wk = it.wk; hk = it.hk;
        row_stride = (ptrdiff_t)it.src_stride[which];
        g.img = reinterpret_cast<const T*>(it.src[which]);
        g.dst = out + it.offI + (size_t)which * wk * hk;
    } else {
        g.img = srow(src, blockIdx.z, img_stride);
        g.dst = out + (size_t)blockIdx.z * wk * hk;
    }
    return true;
}

// Same-size level (k = 0), generic: one thread per pixel, no resample.
template <bool HET, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_same(const T* __restrict__ src, ptrdiff_t row_stride,
                                                    ptrdiff_t img_stride, int W, int H, nsof_blur_taps t,
                                                    float* __restrict__ out, const nsof_het_item* __restrict__ items,
                                                    int want_flag)
{
    __shared__ float s_tk[NSOF_MAX_BLUR_TAPS];
    stage_taps(s_tk, t);
    __syncthreads();
    auto tk = [&](int j) { return s_tk[j]; };
    PrepImg<T> g;
    int wk = W, hk = H;
    if (!prep_geom<HET>(g, src, row_stride, img_stride, W, H, wk, hk, out, items, want_flag)) return;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const T* img = g.img;
    auto hv = [&](int rr) {
        const T* rowp = srow(img, reflect101(rr, H), row_stride);
        return row_filter<0, FMA>(tk, t.ksize, x, [&](int c) { return px(rowp + reflect101(c, W)); });
    };
    g.dst[(size_t)y * W + x] = col_filter<0, FMA>(tk, t.ksize, y, hv);
}

// Same-size level with the 3-tap kernel (every level 0): a lane owns 4 adjacent pixels of 8 consecutive rows.
// One aligned dword load per row; the two bytes outside the dword come from the neighbouring lanes
// (the wave's edge lanes fetch theirs from memory); row-filter results are shared between the three
// output rows that use them; 16-B stores.  Requires 4-byte aligned rows (else k_prep_same).
// T = float / 16-bit: the lane's 4 pixels are one aligned 16-B / 8-B load per row (rows aligned to that, else
// k_prep_same), the two outside values come from the neighbouring lanes the same way.
constexpr int PREP0_ROWS = 8;
template <bool HET, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_same3_vec(const T* __restrict__ src, ptrdiff_t row_stride,
                                                         ptrdiff_t img_stride, int W, int H, float k0, float k1,
                                                         float* __restrict__ out,
                                                         const nsof_het_item* __restrict__ items)
{
    PrepImg<T> g;
    int wk = W, hk = H;
    if (!prep_geom<HET>(g, src, row_stride, img_stride, W, H, wk, hk, out, items, NSOF_HET_VEC0)) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = (blockIdx.x * 64 + lane) * 4;                  // first of this lane's 4 pixels
    const int y0 = (blockIdx.y * 4 + wave) * PREP0_ROWS;
    if (y0 >= H || blockIdx.x * 256 >= W) return;                 // wave-uniform
    const bool live = x < W;
    const int xl = live ? x : 0;                                  // dead lanes still take part in the shuffles
    const T* img = g.img;
    float* dst = g.dst;

    auto hrow = [&](int rr, float (&h)[4]) {                      // row filter of source row rr (reflected)
        const T* rowp = srow(img, reflect101(rr, H), row_stride);
        float s0, s1, s2, s3, sl, sr;
        // (8-bit: the neighbours' raw dwords are exchanged and converted after; in the quad form below, which exchanges
        // converted pixels, the level-0 launch of 64 1080p frames measured 133.5 us against 130.2 .. 131.7)
        if constexpr (kU8<T>) {
            const unsigned v = *reinterpret_cast<const unsigned*>(rowp + xl);
            unsigned lft = __shfl_up(v, 1) >> 24, rgt = __shfl_down(v, 1) & 0xffu;
            if (lane == 0 || x == 0) lft = rowp[reflect101(xl - 1, W)];
            if (lane == 63 || x + 4 >= W) rgt = rowp[reflect101(xl + 4, W)];
            s0 = (float)(v & 0xffu); s1 = (float)((v >> 8) & 0xffu); s2 = (float)((v >> 16) & 0xffu);
            s3 = (float)(v >> 24); sl = (float)lft; sr = (float)rgt;
        } else {
            const PxQuad<T> v = *reinterpret_cast<const PxQuad<T>*>(rowp + xl);
            s0 = quad_el<T>(v, 0); s1 = quad_el<T>(v, 1); s2 = quad_el<T>(v, 2); s3 = quad_el<T>(v, 3);
            sl = __shfl_up(s3, 1);
            sr = __shfl_down(s0, 1);
            if (lane == 0 || x == 0) sl = px(rowp + reflect101(xl - 1, W));
            if (lane == 63 || x + 4 >= W) sr = px(rowp + reflect101(xl + 4, W));
        }
        h[0] = nsof_madd<FMA>(sl + s1, k1, s0 * k0);
        h[1] = nsof_madd<FMA>(s0 + s2, k1, s1 * k0);
        h[2] = nsof_madd<FMA>(s1 + s3, k1, s2 * k0);
        h[3] = nsof_madd<FMA>(s2 + sr, k1, s3 * k0);
    };
    float hm[4], h0[4], hp[4];
    hrow(y0 - 1, hm);
    hrow(y0, h0);
#pragma unroll
    for (int q = 0; q < PREP0_ROWS; q++) {
        const int y = y0 + q;
        if (y >= H) break;                                        // wave-uniform
        hrow(y + 1, hp);
        if (live) {
            float4 o;
            o.x = nsof_madd<FMA>(hm[0] + hp[0], k1, h0[0] * k0);
            o.y = nsof_madd<FMA>(hm[1] + hp[1], k1, h0[1] * k0);
            o.z = nsof_madd<FMA>(hm[2] + hp[2], k1, h0[2] * k0);
            o.w = nsof_madd<FMA>(hm[3] + hp[3], k1, h0[3] * k0);
            nsof_store_stream4(dst + (size_t)y * W + x, o.x, o.y, o.z, o.w);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { hm[i] = h0[i]; h0[i] = hp[i]; }
    }
}

// Resampled level for EXACT decimation by S = 2, 4, 8 (W = S*wk, H = S*hk, W % 16 == 0: the pyr_scale 0.5 pyramids
// of 1080p/4K frames).  The thread-per-output kernels below issue dozens of narrow loads per output pixel and are
// bound by the L1's 4 lanes/cycle; here a lane owns 16 adjacent source columns (16/S output pixels) and walks down
// the output rows of its segment:
//   * one aligned 16-B load per source row + one halo load per side (the image's own edge reflects out of the
//     lane's 16 bytes, no extra load),
//   * the row filter is evaluated only at the columns the resize samples (S*j + S/2 - 1 and the next one), once
//     per source row, and kept in a register ring of RING >= KS + 1 rows (static slots: the walk is unrolled
//     over RING / S steps),
//   * column filter at the two sampled rows, then resize's 2x2 blend (all four weights are exactly 0.5).
// Same operation order as the other prep kernels (row_filter / col_filter), so the output is bit-identical.
// The walk of one wave: column group `bx * 64 + lane`, output rows [seg * seg_rows, (seg + 1) * seg_rows) of image z.
// T = float / 16-bit: the same walk over CW pixels per lane (CW / 4 aligned 16-B / 8-B loads per row, HB / 4 per halo
// side; rows 16- / 8-byte aligned), prefetching one output row ahead only at S = 2 for float -- a raw f32 row is four
// times the registers of an 8-bit one -- and at S <= 4 for 16-bit, as for 8-bit.  Every load stays inside its row
// (halo_l / halo_r below).
template <int S, int KS, int CW, typename T, bool FMA>
__device__ __forceinline__ void prep_decim_body(const T* __restrict__ src, ptrdiff_t row_stride, ptrdiff_t img_stride,
                                                int W, int H, int wk, int hk, int seg_rows, const nsof_blur_taps& t,
                                                float* __restrict__ out, int bx, int seg, int z)
{
    // CW = source columns per lane: 16 (one 16-B load per row) when W % 16 == 0, else 8 (W % 8 == 0, e.g. the
    // 1080-wide portrait frames of the reference's grasp sequence)
    constexpr int R = KS / 2, NPX = CW / S, NC = 2 * NPX;
    constexpr int RING = (KS + 1 + S - 1) / S * S, U = RING / S;
    constexpr int HB = (R + 3) / 4 * 4, HD = HB / 4;          // halo bytes / dwords per side
    constexpr int WIN = HB + CW + HB;
    static_assert(NPX >= 1, "lane narrower than one output pixel");
    const int lane = threadIdx.x & 63;
    const int TG = bx * 64 + lane;                             // CW-column group
    const int dy0 = seg * seg_rows;
    if (dy0 >= hk) return;                                     // wave-uniform
    const int dy1 = min(dy0 + seg_rows, hk);
    const bool live = CW * TG < W;
    const int xc0 = live ? CW * TG : 0;
    const bool edge_l = xc0 == 0, edge_r = xc0 + CW >= W;
    const T* img = srow(src, z, img_stride);
    float* dst = out + (size_t)z * wk * hk;
    auto tk = [&](int j) { return t.k[j]; };                   // static index after unrolling

    float ring[RING][NC];

    // A source row as loaded: the lane's CW bytes + HB halo bytes per side.  fetch() only issues the loads, filt()
    // evaluates the row filter at this lane's sampled columns -> ring[slot]; between the two a row can stay in flight
    // while the rows before it are filtered (S <= 4: the rows of the NEXT output row are fetched before this one's are
    // used -- with one output row's 2 or 4 source rows in flight per wave the kernel waited for memory half the time).
    using Q = PxQuad<T>;   // 4 pixels: a dword / an 8-B / a 16-B vector
    struct Raw {
        Q cw[CW / 4], hl[HD], hr[HD];
    };
    // Halo quad d of a side covers columns [xc0 - HB + 4d, +4) (left) / [xc0 + CW + 4d, +4) (right): whole quads, as
    // W % CW == 0.  A lane reads at most R + 1 - S/2 (<= 6) columns beyond its segment, and the edge lanes reflect into
    // their own pixels and their inner halo.  With HB <= CW the halos of every lane that is not at the image edge lie
    // inside the row, and the edge lanes load theirs from their own segment (values unused).  With HB > CW (19 taps at
    // S = 8 on 8-column lanes) the lane next to an edge would reach over the row's end by HB - CW columns: a quad that
    // lies outside the row is loaded from rowp instead (its values are never used).  So every load stays in the row.
    auto halo_l = [&](const T* rowp, int d) -> const T* {
        if constexpr (HB > CW) return xc0 - HB + 4 * d >= 0 ? rowp - HB + 4 * d : rowp;
        else return (edge_l ? rowp : rowp - HB) + 4 * d;
    };
    auto halo_r = [&](const T* rowp, int d) -> const T* {
        if constexpr (HB > CW) return xc0 + CW + 4 * d + 4 <= W ? rowp + CW + 4 * d : rowp;
        else return (edge_r ? rowp + (kU8<T> ? 0 : CW - HB) : rowp + CW) + 4 * d;
    };
    auto fetch = [&](int r, Raw& q) {
        const T* rowp = srow(img, reflect101(r, H), row_stride) + xc0;
        if constexpr (kU8<T> && CW == 16) {   // 8-bit: the lane's CW bytes are one 16-B / 8-B load
            const uint4 c = *reinterpret_cast<const uint4*>(rowp);
            q.cw[0] = c.x; q.cw[1] = c.y; q.cw[2] = c.z; q.cw[3] = c.w;
        } else if constexpr (kU8<T>) {
            const uint2 c = *reinterpret_cast<const uint2*>(rowp);
            q.cw[0] = c.x; q.cw[1] = c.y;
        } else {
#pragma unroll
            for (int d = 0; d < CW / 4; d++) q.cw[d] = reinterpret_cast<const Q*>(rowp)[d];
        }
#pragma unroll
        for (int d = 0; d < HD; d++) {
            q.hl[d] = *reinterpret_cast<const Q*>(halo_l(rowp, d));
            q.hr[d] = *reinterpret_cast<const Q*>(halo_r(rowp, d));
        }
    };
    auto filt = [&](const Raw& q, float (&dstrow)[NC]) {
        float raw[WIN];   // window [xc0 - HB, xc0 + CW + HB) as loaded
#pragma unroll
        for (int b = 0; b < HB; b++) {
            raw[b] = quad_el<T>(q.hl[b >> 2], b & 3);
            raw[HB + CW + b] = quad_el<T>(q.hr[b >> 2], b & 3);
        }
#pragma unroll
        for (int b = 0; b < CW; b++) raw[HB + b] = quad_el<T>(q.cw[b >> 2], b & 3);
        float fb[WIN];
#pragma unroll
        for (int b = 0; b < CW; b++) fb[HB + b] = raw[HB + b];
#pragma unroll
        for (int b = 0; b < HB; b++) {
            // left halo byte b is column xc0 - HB + b; at the image edge (xc0 == 0) it reflects to column HB - b
            fb[b] = edge_l ? raw[HB + (HB - b)] : raw[b];
            // right halo byte b is column xc0 + CW + b; at the edge (xc0 + CW == W) it reflects to column W - 2 - b
            fb[HB + CW + b] = edge_r ? raw[HB + CW - 2 - b] : raw[HB + CW + b];
        }
#pragma unroll
        for (int n = 0; n < NC; n++) {
            const int off = HB + S * (n >> 1) + S / 2 - 1 + (n & 1);
            dstrow[n] = row_filter<KS, FMA>(tk, KS, off, [&](int q2) { return fb[q2]; });
        }
    };
    auto load_row = [&](int r, float (&dstrow)[NC]) {
        Raw q;
        fetch(r, q);
        filt(q, dstrow);
    };
    constexpr bool PF = S <= (sizeof(T) <= 2 ? 4 : 2);   // prefetch one output row ahead

    // relative row index rel = r - base, base = first row needed by output row dy0; slot = rel % RING
    const int base = S * dy0 + S / 2 - 1 - R;
#pragma unroll
    for (int i = 0; i <= KS - S; i++) load_row(base + i, ring[i % RING]);

    Raw nx[PF ? S : 1];
    if constexpr (PF) {
#pragma unroll
        for (int i = 0; i < S; i++) fetch(base + KS - S + 1 + i, nx[i]);
    }
    for (int g = 0; dy0 + g * U < dy1; g++) {
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int dy = dy0 + g * U + u;
            if (dy >= dy1) break;                               // wave-uniform
            if constexpr (PF) {
                Raw cu[S];
#pragma unroll
                for (int i = 0; i < S; i++) cu[i] = nx[i];
                // the next output row's source rows (beyond the segment: reflected rows of the image, never used)
#pragma unroll
                for (int i = 0; i < S; i++) fetch(base + S * (g * U + u + 1) + KS - S + 1 + i, nx[i]);
#pragma unroll
                for (int i = 0; i < S; i++) filt(cu[i], ring[(S * u + KS - S + 1 + i) % RING]);
            } else {
#pragma unroll
                for (int i = 0; i < S; i++) {
                    load_row(base + S * (g * U + u) + KS - S + 1 + i, ring[(S * u + KS - S + 1 + i) % RING]);
                }
            }
            if (live) {
                float o[NPX];
#pragma unroll
                for (int j = 0; j < NPX; j++) {
                    auto col = [&](int n, int centre) {
                        return col_filter<KS, FMA>(tk, KS, centre, [&](int q) { return ring[(S * u + q) % RING][n]; });
                    };
                    const float B00 = col(2 * j, R), B01 = col(2 * j + 1, R);
                    const float B10 = col(2 * j, R + 1), B11 = col(2 * j + 1, R + 1);
                    const float t0 = B00 * 0.5f + B01 * 0.5f;
                    const float t1 = B10 * 0.5f + B11 * 0.5f;
                    o[j] = t0 * 0.5f + t1 * 0.5f;
                }
                nsof_store_stream_n(dst + (size_t)dy * wk + NPX * TG, o);
            }
        }
    }
}

template <int S, int KS, int CW, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_decim(const T* __restrict__ src, ptrdiff_t row_stride,
                                                     ptrdiff_t img_stride, int W, int H, int wk, int hk, int seg_rows,
                                                     nsof_blur_taps t, float* __restrict__ out)
{
    prep_decim_body<S, KS, CW, T, FMA>(src, row_stride, img_stride, W, H, wk, hk, seg_rows, t, out, blockIdx.x,
                                       blockIdx.y * 4 + (threadIdx.x >> 6), blockIdx.z);
}

// Levels 1, 2, 3 of a pyr_scale 0.5 pyramid in ONE launch: twelve waves per workgroup, four per level, all over the same
// 1024 (512) source columns and the same 4 x 96 source rows -- each level smooths the FULL-RES frame, so run as three
// launches the frame crossed the fabric three times; side by side the second and third reader find its rows in the cache.
// Same walks, same bits (prep_decim_body).
struct Decim3 {
    nsof_blur_taps t[3];
    float* out[3];
    int seg_rows[3];
};
template <int CW, typename T, bool FMA>
__global__ __launch_bounds__(768) void k_prep_decim3(const T* __restrict__ src, ptrdiff_t row_stride,
                                                      ptrdiff_t img_stride, int W, int H, Decim3 d)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int seg = blockIdx.y * 4 + (wave & 3);
    if (wave < 4)
        prep_decim_body<2, 3, CW, T, FMA>(src, row_stride, img_stride, W, H, W / 2, H / 2, d.seg_rows[0], d.t[0], d.out[0], blockIdx.x, seg, blockIdx.z);
    else if (wave < 8)
        prep_decim_body<4, 9, CW, T, FMA>(src, row_stride, img_stride, W, H, W / 4, H / 4, d.seg_rows[1], d.t[1], d.out[1], blockIdx.x, seg, blockIdx.z);
    else
        prep_decim_body<8, 19, CW, T, FMA>(src, row_stride, img_stride, W, H, W / 8, H / 8, d.seg_rows[2], d.t[2], d.out[2], blockIdx.x, seg, blockIdx.z);
}

// Resampled level, generic fallback: one thread per destination pixel, no data sharing.
template <bool HET, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_naive(const T* __restrict__ src, ptrdiff_t row_stride,
                                                     ptrdiff_t img_stride, int W, int H, int wk, int hk,
                                                     double scale_x, double scale_y, nsof_blur_taps t,
                                                     float* __restrict__ out, const nsof_het_item* __restrict__ items)
{
    __shared__ float s_tk[NSOF_MAX_BLUR_TAPS];
    stage_taps(s_tk, t);
    __syncthreads();
    auto tk = [&](int j) { return s_tk[j]; };
    PrepImg<T> g;
    prep_geom<HET>(g, src, row_stride, img_stride, W, H, wk, hk, out, items, -1);
    if constexpr (HET) { scale_x = inv_scale(wk, W); scale_y = inv_scale(hk, H); }
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= wk || dy >= hk) return;
    const T* img = g.img;
    const LinTap tx = lin_tap_x(dx, scale_x, W), ty = lin_tap_y(dy, scale_y, H);
    auto blur = [&](int rr, int cc) {
        auto hv = [&](int q) {
            const T* rowp = srow(img, reflect101(q, H), row_stride);
            return row_filter<0, FMA>(tk, t.ksize, cc, [&](int c) { return px(rowp + reflect101(c, W)); });
        };
        return col_filter<0, FMA>(tk, t.ksize, rr, hv);
    };
    g.dst[(size_t)dy * wk + dx] = lin_blend<FMA>(blur(ty.i0, tx.i0), blur(ty.i0, tx.i1), blur(ty.i1, tx.i0),
                                               blur(ty.i1, tx.i1), tx.w1, ty.w1);
}

// Resampled level, LDS-tiled: a 32x8 destination tile per 256-thread block.
//   phase 1: source footprint (with blur halo, borders reflected) -> LDS as T (coalesced row segments)
//   phase 2: row filter only at the 2 source columns each destination column samples
//   phase 3: column filter only at the 2 source rows each destination row samples
//   phase 4: bilinear blend (horizontal first, then vertical, as resize does)
// KS = compile-time kernel size (3, 5, 9, 19: pyr_scale 0.5 / 0.6 with up to 3 levels) or 0 = runtime.
constexpr int PREP_TW = 32, PREP_TH = 8;
constexpr int tiled_ks(int ksize) { return ksize == 9 || ksize == 19 ? ksize : 0; }   // the KS a kernel size takes
template <int KS, bool HET, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_tiled(const T* __restrict__ src, ptrdiff_t row_stride,
                                                     ptrdiff_t img_stride, int W, int H, int wk, int hk,
                                                     double scale_x, double scale_y, int rw_cap, int rh_cap,
                                                     nsof_blur_taps t, float* __restrict__ out,
                                                     const nsof_het_item* __restrict__ items)
{
    PrepImg<T> g;
    prep_geom<HET>(g, src, row_stride, img_stride, W, H, wk, hk, out, items, -1);
    if constexpr (HET) {
        scale_x = inv_scale(wk, W);
        scale_y = inv_scale(hk, H);
        if (blockIdx.x * PREP_TW >= wk || blockIdx.y * PREP_TH >= hk) return;   // block-uniform
    }
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* sH = reinterpret_cast<float*>(smem);                 // [rh_cap][2*TW]
    float* sB = sH + (size_t)rh_cap * (2 * PREP_TW);            // [2*TH][2*TW]
    T* sU = reinterpret_cast<T*>(sB + 2 * PREP_TH * 2 * PREP_TW);  // [rh_cap][rw_cap]
    __shared__ int s_c[2 * PREP_TW];   // absolute source column per (dst col, 0/1)
    __shared__ int s_r[2 * PREP_TH];   // absolute source row per (dst row, 0/1)
    __shared__ float s_a[PREP_TW], s_b[PREP_TH];
    __shared__ float s_tk[NSOF_MAX_BLUR_TAPS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ksize = KS ? KS : t.ksize, r = ksize >> 1;
    const int dx0 = blockIdx.x * PREP_TW, dy0 = blockIdx.y * PREP_TH;
    const T* img = g.img;
    auto tk = [&](int j) { return KS ? t.k[j] : s_tk[j]; };   // KS > 0: j is a constant after unrolling

    if (tid < PREP_TW) {
        const LinTap tx = lin_tap_x(min(dx0 + tid, wk - 1), scale_x, W);
        s_c[2 * tid] = tx.i0;
        s_c[2 * tid + 1] = tx.i1;
        s_a[tid] = tx.w1;
    } else if (tid >= 64 && tid < 64 + PREP_TH) {
        const int i = tid - 64;
        const LinTap ty = lin_tap_y(min(dy0 + i, hk - 1), scale_y, H);
        s_r[2 * i] = ty.i0;
        s_r[2 * i + 1] = ty.i1;
        s_b[i] = ty.w1;
    }
    if constexpr (!KS) stage_taps(s_tk, t, 128);   // (threads of the third wave)
    __syncthreads();
    // coordinates are monotone in dx/dy, so the footprint is [first .. last]
    int C0 = s_c[0] - r;
    const int RW0 = s_c[2 * PREP_TW - 1] + r - C0 + 1;
    const int R0 = s_r[0] - r, RH = s_r[2 * PREP_TH - 1] + r - R0 + 1;
    // host sized rw_cap/rh_cap from the same arithmetic (+4 columns of slack for the aligned copy below)
    constexpr int PPD = kPPD<T>;   // integer frames: pixels per dword
    const bool interior = kInt<T> && C0 >= 0 && C0 + RW0 <= W && R0 >= 0 && R0 + RH <= H && (W % PPD) == 0 &&
                          (row_stride & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 3) == 0;
    if (interior) {
        // no border inside the footprint: copy whole aligned dwords (64 lanes x 4 B per wave-instruction)
        const int C0a = C0 & ~(PPD - 1), nd = (C0 + RW0 - C0a + PPD - 1) / PPD;
        C0 = C0a;   // the LDS image now starts at the aligned column
#pragma unroll 4
        for (int rr = wave; rr < RH; rr += 4) {
            const T* rowp = srow(img, R0 + rr, row_stride) + C0a;
            for (int d = lane; d < nd; d += 64)
                *reinterpret_cast<unsigned*>(sU + rr * rw_cap + PPD * d) = *reinterpret_cast<const unsigned*>(rowp + PPD * d);
        }
    } else {
        for (int rr = wave; rr < RH; rr += 4) {          // border tile (and f32 frames): per pixel, BORDER_REFLECT_101
            const T* rowp = srow(img, reflect101(R0 + rr, H), row_stride);
            for (int cc = lane; cc < RW0; cc += 64) sU[rr * rw_cap + cc] = rowp[reflect101(C0 + cc, W)];
        }
    }
    __syncthreads();
    {
        const int cj = s_c[lane] - C0;                // this lane's sampled column, local
#pragma unroll 2
        for (int rr = wave; rr < RH; rr += 4) {
            const T* rowp = sU + rr * rw_cap;
            sH[rr * (2 * PREP_TW) + lane] = row_filter<KS, FMA>(tk, ksize, cj, [&](int c) { return px(rowp + c); });
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = wave; q < 2 * PREP_TH; q += 4)       // 16 sampled rows x 64 sampled columns
        sB[q * (2 * PREP_TW) + lane] =
            col_filter<KS, FMA>(tk, ksize, s_r[q] - R0, [&](int rr) { return sH[rr * (2 * PREP_TW) + lane]; });
    __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    const int dx = dx0 + tx, dy = dy0 + ty;
    if (dx < wk && dy < hk) {
        const float* B0 = sB + (2 * ty) * (2 * PREP_TW) + 2 * tx;
        const float* B1 = B0 + 2 * PREP_TW;
        g.dst[(size_t)dy * wk + dx] = lin_blend<FMA>(B0[0], B0[1], B1[0], B1[1], s_a[tx], s_b[ty]);
    }
}

// Resampled level, direct: one thread per destination pixel, everything in registers, no LDS, no barriers.
// A destination pixel blends the blurred image at 2x2 source positions (rows r0,r1 x columns c0,c1), i.e. it
// needs the row-filtered values H at columns c0 and c1 of the KS+1 source rows r0-R..r1+R; each of those rows
// contributes KS+1 consecutive bytes, fetched as unaligned dwords (L1/L2 resident: the u8 frame is 2 MB).
// More arithmetic than the LDS-tiled variant but no per-tile overhead -- measured 3-6x faster at 1080p.
// Pixels whose footprint leaves the image take a per-byte path with BORDER_REFLECT_101 indexing.
template <int KS, bool HET, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_direct(const T* __restrict__ src, ptrdiff_t row_stride,
                                                      ptrdiff_t img_stride, int W, int H, int wk, int hk,
                                                      double scale_x, double scale_y, nsof_blur_taps t,
                                                      float* __restrict__ out, const nsof_het_item* __restrict__ items)
{
    constexpr int R = KS / 2;
    PrepImg<T> g;
    prep_geom<HET>(g, src, row_stride, img_stride, W, H, wk, hk, out, items, -1);
    if constexpr (HET) { scale_x = inv_scale(wk, W); scale_y = inv_scale(hk, H); }
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= wk || dy >= hk) return;
    const T* img = g.img;
    const LinTap tx = lin_tap_x(dx, scale_x, W), ty = lin_tap_y(dy, scale_y, H);
    const bool fast = window_fast<T, KS + 1>(tx.i0, tx.i1, R, W);
    auto tk = [&](int j) { return t.k[j]; };   // j is a compile-time constant after unrolling

    float H0[KS + 1], H1[KS + 1];   // row filter at columns c0 and c1 of source rows r0 - R .. r0 - R + KS
#pragma unroll
    for (int i = 0; i <= KS; i++) {
        const T* rowp = srow(img, reflect101(ty.i0 - R + i, H), row_stride);
        if (fast) {   // one window of KS + 1 pixels serves both columns
            float b[KS + 1];
            load_window<T, KS + 1>(rowp, tx.i0 - R, b);
            H0[i] = row_filter<KS, FMA>(tk, KS, R, [&](int c) { return b[c]; });
            H1[i] = row_filter<KS, FMA>(tk, KS, R + 1, [&](int c) { return b[c]; });
        } else {
            float b[KS], bb[KS];
            load_window_reflect<T, KS>(rowp, tx.i0 - R, W, b);
            load_window_reflect<T, KS>(rowp, tx.i1 - R, W, bb);
            H0[i] = row_filter<KS, FMA>(tk, KS, R, [&](int c) { return b[c]; });
            H1[i] = row_filter<KS, FMA>(tk, KS, R, [&](int c) { return bb[c]; });
        }
    }
    g.dst[(size_t)dy * wk + dx] = resample_tail<KS, FMA>(
        tk, [&](int q) { return H0[q]; }, [&](int q) { return H1[q]; }, ty.i1 != ty.i0, tx.w1, ty.w1);
}

// Resampled level, walking: thread <-> destination column, a wave walks a segment of destination rows top to bottom.
// The direct kernel above recomputes, for EVERY destination pixel, the row filter of its KS+1 source rows (one or more
// unaligned dword loads each); consecutive destination rows of a column share most of those rows.  Here a thread keeps the
// row-filtered values of its two sampled columns for a window of KS+1 source rows in registers (H0 / H1, shifted as the
// window advances -- by 1 or 2 rows per destination row at pyr_scale 0.6, 4-5 at level 3) and loads / row-filters every
// source row ONCE: 1.7 instead of 4 row evaluations per destination pixel at level 1, 4.6 instead of 10 at level 3.  The
// advance loop is wave-uniform (source rows depend on the destination row only).  Same helper functions and operation
// order as the direct kernel -> bit-identical output.  (This kernel spells its window loads, its tap set-up and its
// resample tail out instead of taking load_window / lin_tap_x / resample_tail: written with them the integer walks
// measured 0.1-0.9 % slower, the 1080p level-3 launch of 64 frames 236.6 us against 234.3 .. 234.6.)  Parameter sets B / C (pyr_scale 0.6):
// levels 1, 2 and 3 (3 / 5 / 9 taps).
// The walk is written for the scalar unit.  Everything that depends on the destination ROW only -- the source rows of
// its window, "has the window's last row entered", the vertical blend weight -- is wave-uniform and lives in SGPRs
// (readfirstlane), so the loop's control flow is scalar branches instead of exec-mask bookkeeping; and whether a lane
// may take the fast window (its KS + 1 pixels lie inside the image) is decided once per WAVE: only the waves that touch
// the left / right image border run the per-pixel reflecting loads.  With a per-lane choice in the loop the kernel spent
// ~240 instructions per source row, most of them mask handling, where the arithmetic needs ~20.
template <int U, int N, class F>
__device__ __forceinline__ void prep_static_slots(F& f)
{
    if constexpr (U < N) {
        if (f(std::integral_constant<int, U>{})) prep_static_slots<U + 1, N>(f);
    }
}

template <int KS, bool WFAST, typename T, bool FMA>
__device__ __forceinline__ void prep_walk_body(const T* __restrict__ img, ptrdiff_t row_stride, int W, int H, int wk, int hk,
                                               double scale_y, int dy0, int dy_end, int dx, bool live, int c0, int c1, bool fast,
                                               float a1, const nsof_blur_taps& t, float* __restrict__ dst)
{
    constexpr int R = KS / 2, NB = KS + 1, PPD = kPPD<T>, ND = (NB + PPD - 1) / PPD;
    const float a0 = 1.f - a1;
    auto tk = [&](int j) { return t.k[j]; };   // j is a compile-time constant after unrolling
    const unsigned coff = (unsigned)(c0 - R);    // pixel offset of this lane's window in a source row (fast lanes)
    // the KS + 1 pixels of source row rr (wave-uniform, any integer: reflected) around this lane's two columns, as raw dwords
    auto load_row = [&](int rr, unsigned (&raw)[ND]) {
        const T* rowp = srow(img, reflect101(rr, H), row_stride);   // scalar
#pragma unroll
        for (int d = 0; d < ND; d++) __builtin_memcpy(&raw[d], rowp + coff + PPD * d, 4);   // unaligned dword loads
    };
    // row-filtered values at columns c0 and c1 from those pixels
    auto filt_row = [&](const unsigned (&raw)[ND], float& h0, float& h1) {
        float b[NB];
#pragma unroll
        for (int d = 0; d < ND; d++)
#pragma unroll
            for (int e = 0; e < PPD; e++)
                if (PPD * d + e < NB) b[PPD * d + e] = px_el<T>(raw[d], e);
        h0 = row_filter<KS, FMA>(tk, KS, R, [&](int c) { return b[c]; });
        h1 = row_filter<KS, FMA>(tk, KS, R + 1, [&](int c) { return b[c]; });
    };
    // border waves: per lane, per byte with BORDER_REFLECT_101 where the window leaves the image
    auto hrow_edge = [&](int rr, float& h0, float& h1) {
        const T* rowp = srow(img, reflect101(rr, H), row_stride);
        if (fast) {
            if constexpr (kInt<T>) {
                unsigned raw[ND];
#pragma unroll
                for (int d = 0; d < ND; d++) __builtin_memcpy(&raw[d], rowp + coff + PPD * d, 4);
                filt_row(raw, h0, h1);
            } else {   // f32: the NB values around c0 straight from the row
                float b[NB];
#pragma unroll
                for (int j = 0; j < NB; j++) b[j] = rowp[coff + j];
                h0 = row_filter<KS, FMA>(tk, KS, R, [&](int c) { return b[c]; });
                h1 = row_filter<KS, FMA>(tk, KS, R + 1, [&](int c) { return b[c]; });
            }
        } else {
            float b[NB], bb[NB];
#pragma unroll
            for (int j = 0; j < KS; j++) {
                b[j] = px(rowp + reflect101(c0 - R + j, W));
                bb[j] = px(rowp + reflect101(c1 - R + j, W));
            }
            h0 = row_filter<KS, FMA>(tk, KS, R, [&](int c) { return b[c]; });
            h1 = row_filter<KS, FMA>(tk, KS, R, [&](int c) { return bb[c]; });
        }
    };
    // destination row dy -> its two source rows and the vertical weight, all wave-uniform (SGPRs)
    auto row_coord = [&](int dy, int& r0, int& r1, float& b1) {
        int sy;
        float bv;
        lin_coord_y(dy, scale_y, sy, bv);
        sy = __builtin_amdgcn_readfirstlane(sy);
        b1 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, bv)));
        r0 = clampi(sy, 0, H - 1);
        r1 = clampi(sy + 1, 0, H - 1);
    };
    // The row-filtered pairs of the KS + 1 newest source rows live in a register ring with STATIC slots: source rows are
    // taken strictly in order, row rstart + i into slot i % NB (the walk is unrolled NB times), and a destination row is
    // emitted when the last row of its window, r0 + R + 1, has just entered -- its window rows then sit at the slots
    // (u + 1 + q) % NB, q = 0..KS, known at compile time.  (Windows of consecutive destination rows overlap -- the launcher
    // takes this kernel only while a destination step is shorter than the ring -- so no source row is filtered in vain.)
    float H0[NB], H1[NB];
    int dy = dy0, r0, r1;
    float b1;
    row_coord(dy, r0, r1, b1);
    const int rstart = r0 - R;
    int last = r0 - R + KS;                                        // the source row that completes the window of dy
    // (interior waves) the raw bytes of the NEXT block of KS + 1 source rows are requested before this block is filtered:
    // a wave then has a block of loads in flight instead of waiting for every row's load on its own
    unsigned cur[NB][ND], nxt[NB][ND];
    if constexpr (WFAST) {
#pragma unroll
        for (int u = 0; u < NB; u++) load_row(rstart + u, cur[u]);
    }
    for (int rb = 0; dy < dy_end && rb <= H + 2 * NB; rb += NB) {   // (bounded: at most H + KS + 1 source rows are walked)
        if constexpr (WFAST) {
#pragma unroll
            for (int u = 0; u < NB; u++) load_row(rstart + rb + NB + u, nxt[u]);   // rows beyond the segment: reflected, unused
        }
        // (expanded at compile time: with 10 slots a `#pragma unroll` loop stayed rolled and indexed the ring dynamically)
        auto slot = [&](auto uc) -> bool {
            constexpr int u = decltype(uc)::value;
            if (dy >= dy_end) return false;                        // scalar
            const int r = rstart + rb + u;
            if constexpr (WFAST) filt_row(cur[u], H0[u], H1[u]);
            else hrow_edge(r, H0[u], H1[u]);
            if (r == last) {                                       // scalar
                const float b0 = 1.f - b1;
                const float B00 = col_filter<KS, FMA>(tk, KS, R, [&](int q) { return H0[(u + 1 + q) % NB]; });
                const float B01 = col_filter<KS, FMA>(tk, KS, R, [&](int q) { return H1[(u + 1 + q) % NB]; });
                float B10 = B00, B11 = B01;
                if (r1 != r0) {
                    B10 = col_filter<KS, FMA>(tk, KS, R + 1, [&](int q) { return H0[(u + 1 + q) % NB]; });
                    B11 = col_filter<KS, FMA>(tk, KS, R + 1, [&](int q) { return H1[(u + 1 + q) % NB]; });
                }
                const float t0 = nsof_madd<FMA>(B00, a0, B01 * a1);
                const float t1 = nsof_madd<FMA>(B10, a0, B11 * a1);
                if (live) __builtin_nontemporal_store(nsof_madd<FMA>(t0, b0, t1 * b1), dst + (size_t)dy * wk + dx);
                dy++;
                if (dy < dy_end) {
                    row_coord(dy, r0, r1, b1);
                    last = r0 - R + KS;
                }
            }
            return true;
        };
        prep_static_slots<0, NB>(slot);
        if constexpr (WFAST) {
#pragma unroll
            for (int u = 0; u < NB; u++)
#pragma unroll
                for (int d = 0; d < ND; d++) cur[u][d] = nxt[u][d];
        }
    }
}

// T = float: every wave takes the per-lane form (prep_walk_body<KS, false>): a block of KS + 1 raw f32 rows in flight
// would be (KS + 1)^2 registers per lane.  16-bit rows take the block form at twice the 8-bit registers.
template <int KS, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_walk(const T* __restrict__ src, ptrdiff_t row_stride,
                                                    ptrdiff_t img_stride, int W, int H, int wk, int hk, double scale_x,
                                                    double scale_y, int seg_rows, nsof_blur_taps t, float* __restrict__ out)
{
    constexpr int R = KS / 2, NB = KS + 1, PPD = kPPD<T>, ND = (NB + PPD - 1) / PPD;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int dy0 = (blockIdx.y * 4 + wave) * seg_rows;
    if (dy0 >= hk) return;                                        // wave-uniform
    const int dy_end = min(dy0 + seg_rows, hk);
    const int dxr = blockIdx.x * 64 + lane;
    const bool live = dxr < wk;
    const int dx = live ? dxr : wk - 1;
    const T* img = srow(src, blockIdx.z, img_stride);
    float* dst = out + (size_t)blockIdx.z * wk * hk;
    int sx;
    float a1;
    lin_coord_x(dx, scale_x, W, sx, a1);
    const int c0 = sx, c1 = min(sx + 1, W - 1);
    const bool fast = c0 - R >= 0 && c0 - R + PPD * ND <= W && c1 == c0 + 1;
    if (kInt<T> && __all(fast))
        prep_walk_body<KS, kInt<T>, T, FMA>(img, row_stride, W, H, wk, hk, scale_y, dy0, dy_end, dx, live, c0, c1, true, a1, t, dst);
    else
        prep_walk_body<KS, false, T, FMA>(img, row_stride, W, H, wk, hk, scale_y, dy0, dy_end, dx, live, c0, c1, fast, a1, t, dst);
}

// Resampled level, two passes (kernel sizes 9 and 19: levels 2 and 3 of the reference's parameter sets).
// The destination samples only 2 source columns per destination column and 2 source rows per destination row,
// so the separable blur is evaluated only there:
//   pass A  k_prep_rows  thread <-> (source row, sampled column): KS-tap row filter -> HA [n][H][2*wk] f32
//   pass B  k_prep_cols  thread <-> destination pixel: KS-tap column filter at its 2 rows x 2 columns of HA
//                        (reflected rows), then the bilinear blend (horizontal first, as resize does).
// Both are plain thread-per-output kernels (no LDS, no barriers, full occupancy); HA is 2-4 MB per frame and
// is re-read from L2/MALL.  Same operation order as the tiled/direct kernels (bit-identical results).
constexpr int PREPA_ROWS = 8;
template <int KS, typename T, bool FMA>
__global__ __launch_bounds__(256) void k_prep_rows(const T* __restrict__ src, ptrdiff_t row_stride,
                                                    ptrdiff_t img_stride, int W, int H, int wk, double scale_x,
                                                    nsof_blur_taps t, float* __restrict__ HA)
{
    constexpr int R = KS / 2;
    const int j = blockIdx.x * 64 + (threadIdx.x & 63);
    const int rbase = (blockIdx.y * 4 + (threadIdx.x >> 6)) * PREPA_ROWS;
    if (j >= 2 * wk || rbase >= H) return;
    const LinTap tx = lin_tap_x(j >> 1, scale_x, W);
    const int c = (j & 1) ? tx.i1 : tx.i0;
    const bool fast = window_fast<T, KS>(c, R, W);
    auto tk = [&](int q) { return t.k[q]; };
    const T* img = srow(src, blockIdx.z, img_stride);
    float* dst = HA + ((size_t)blockIdx.z * H) * (2 * wk) + j;
#pragma unroll 2
    for (int q = 0; q < PREPA_ROWS; q++) {
        const int r = rbase + q;
        if (r >= H) break;
        const T* rowp = srow(img, r, row_stride);
        float b[KS];
        if (fast) load_window<T, KS>(rowp, c - R, b);
        else load_window_reflect<T, KS>(rowp, c - R, W, b);
        dst[(size_t)r * (2 * wk)] = row_filter<KS, FMA>(tk, KS, R, [&](int i) { return b[i]; });
    }
}

template <int KS, bool FMA>
__global__ __launch_bounds__(256) void k_prep_cols(const float* __restrict__ HA, int W, int H, int wk, int hk,
                                                    double scale_x, double scale_y, nsof_blur_taps t,
                                                    float* __restrict__ out)
{
    constexpr int R = KS / 2;
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= wk || dy >= hk) return;
    const LinTap tx = lin_tap_x(dx, scale_x, W), ty = lin_tap_y(dy, scale_y, H);   // (of tx, only the weight)
    auto tk = [&](int q) { return t.k[q]; };
    const float2* Hz = reinterpret_cast<const float2*>(HA) + ((size_t)blockIdx.z * H) * wk + dx;
    float2 Hv[KS + 1];
#pragma unroll
    for (int i = 0; i <= KS; i++) Hv[i] = Hz[(size_t)reflect101(ty.i0 - R + i, H) * wk];
    out[((size_t)blockIdx.z * hk + dy) * wk + dx] = resample_tail<KS, FMA>(
        tk, [&](int q) { return Hv[q].x; }, [&](int q) { return Hv[q].y; }, ty.i1 != ty.i0, tx.w1, ty.w1);
}

}  // namespace

// =========================================================================================
// launchers
// =========================================================================================
namespace {
// ---- sizing ---------------------------------------------------------------------------------------------------------
// Dynamic LDS of k_prep_tiled for source steps (scale_x, scale_y) per destination pixel: row-filtered rows
// [rh_cap][2 TW] and blurred samples [2 TH][2 TW] as f32, then a tile's source footprint [rh_cap][rw_cap] in pixels of
// px_bytes.  The kernel derives the footprint from the same arithmetic (+4 columns of slack for its aligned copy).
struct TiledLds {
    int rw_cap, rh_cap;
    size_t bytes;
};
TiledLds tiled_lds(double scale_x, double scale_y, int ksize, size_t px_bytes)
{
    const int r = ksize / 2;
    TiledLds l;
    l.rw_cap = ((int)ceil(PREP_TW * scale_x) + 2 * r + 8 + 3) / 4 * 4;
    l.rh_cap = (int)ceil(PREP_TH * scale_y) + 2 * r + 4;
    l.bytes = sizeof(float) * ((size_t)l.rh_cap * 2 * PREP_TW + 2 * PREP_TH * 2 * PREP_TW) + (size_t)l.rh_cap * l.rw_cap * px_bytes;
    return l;
}
// Rows of a wave's segment in the walking kernels: `rows`, stepped down by `shorter` while it is above min_rows and the
// launch (waves_x waves across, n_img images of total_rows rows) has fewer than want_waves waves.  A segment re-runs
// ~KS + 1 source rows of warm-up, which only matters when the GPU is full anyway.
template <class Shorter>
int segment_rows(int rows, int min_rows, long waves_x, int total_rows, int n_img, long want_waves, Shorter shorter)
{
    while (rows > min_rows && waves_x * ((total_rows + rows - 1) / rows) * n_img < want_waves) rows = shorter(rows);
    return rows;
}
// k_prep_tiled<tiled_ks(ksize), HET, T, FMA> over `grid`; more than 64 KB of LDS (work lists of 16-bit frames) is opted in.
template <bool HET, typename T, bool FMA>
int launch_tiled(nsof_ctx* ctx, dim3 grid, const TiledLds& l, const T* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W,
                 int H, int wk, int hk, double scale_x, double scale_y, const nsof_blur_taps& taps, float* out,
                 const nsof_het_item* d_items)
{
    int rc = NSOF_OK;
    nsof_with_int<0, 19>(tiled_ks(taps.ksize), [&](auto ks) {
        constexpr int KS = decltype(ks)::value;
        if constexpr (KS == tiled_ks(KS)) {
            rc = [&]() -> int {
                auto kern = k_prep_tiled<KS, HET, T, FMA>;
                if (l.bytes > 64 * 1024)
                    NSOF_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes));
                hipLaunchKernelGGL(kern, grid, dim3(256), l.bytes, ctx->stream, src, row_stride, img_stride, W, H, wk, hk, scale_x,
                                   scale_y, l.rw_cap, l.rh_cap, taps, out, d_items);
                return NSOF_OK;
            }();
        }
    });
    return rc;
}
dim3 tiled_grid(int wk, int hk, int n) { return dim3((wk + PREP_TW - 1) / PREP_TW, (hk + PREP_TH - 1) / PREP_TH, n); }

// Levels 1..3 of a pyr_scale 0.5 pyramid in one launch (k_prep_decim3).  Returns NSOF_EUNSUPPORTED without launching
// when the frames do not decimate exactly by 8 (or are not aligned for the vector walks): the caller then runs the
// levels one by one.  out[k - 1]: level k's images, [n_img][H >> k][W >> k].
template <typename T, bool FMA>
int prep_decim3_impl(nsof_ctx* ctx, int n_img, const T* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W, int H,
                     const nsof_blur_taps* taps, float* const* out)
{
    // 16-bit frames take 8-column lanes: with 16 the three walks need 175 registers more than the 168 a wave has here
    const int CWL = (W & 15) == 0 && kU8<T> ? 16 : 8;
    const int AL = kU8<T> ? CWL : 8;   // the walks' row loads: a lane's CWL bytes (u8) / 8-byte quads (16-bit)
    const bool ok = (W & 7) == 0 && (H & 7) == 0 && W >= 64 && H > 19 && (row_stride % AL) == 0 && (img_stride % AL) == 0 &&
                    (reinterpret_cast<uintptr_t>(src) % AL) == 0 && taps[0].ksize == 3 && taps[1].ksize == 9 &&
                    taps[2].ksize == 19 && n_img <= 65535;
    if (!ok) return NSOF_EUNSUPPORTED;
    nsof_prof_scope ps(ctx, NSOF_K_PREP);
    Decim3 d;
    for (int k = 0; k < 3; k++) {
        d.t[k] = taps[k];
        d.out[k] = out[k];
    }
    // a wave's segment covers the same 96 source rows at every level (48 / 24 / 12 output rows: multiples of the walks'
    // unroll counts 2 / 3 / 3); few images: shorter segments, down to 24 source rows, until there are ~1000 waves
    const long waves_x = (W / CWL + 63) / 64;
    const int src_rows = segment_rows(96, 24, waves_x, H, n_img, 1024, [](int rows) { return rows - 24; });
    d.seg_rows[0] = src_rows / 2;
    d.seg_rows[1] = src_rows / 4;
    d.seg_rows[2] = src_rows / 8;
    const int nseg = (H / 8 + d.seg_rows[2] - 1) / d.seg_rows[2];
    dim3 grid((unsigned)waves_x, (nseg + 3) / 4, n_img);
    nsof_with_int<1, 2>(CWL / 8, [&](auto c) {
        constexpr int CW = 8 * decltype(c)::value;
        if constexpr (CW == 8 || kU8<T>)
            hipLaunchKernelGGL((k_prep_decim3<CW, T, FMA>), grid, dim3(768), 0, ctx->stream, src, row_stride, img_stride, W, H, d);
    });
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// ---- one uniform level: the route, then its launch -------------------------------------------------------------------
enum PrepRoute {
    ROUTE_SAME3_VEC,   // same size, 3 taps, rows aligned for 4-pixel vector loads
    ROUTE_SAME,        // same size, anything else
    ROUTE_DECIM,       // exact decimation by 2 / 4 / 8 with the kernel sizes the pyr_scale 0.5 pyramid produces
    ROUTE_WALK,        // 3 / 5 / 9 taps while consecutive destination rows share source rows
    ROUTE_DIRECT,      // 3 / 5 taps otherwise (larger kernels: registers run out)
    ROUTE_ROWS_COLS,   // 19 taps: two passes
    ROUTE_TILED,       // what fits the LDS budget
    ROUTE_NAIVE        // upscaling, or a footprint too large for the LDS
};
constexpr int decim_lane_cols(int W) { return (W & 15) == 0 ? 16 : 8; }   // source columns per lane of k_prep_decim

// The kernel a level takes, by precedence.  The measurements that set the order (MI355X, 1080p):
//   walk over direct, per 128-image launch at pyr_scale 0.6: level 1 (3 taps) 637 -> 334 us, level 2 (5 taps) 403 ->
//     266 us; per 256 images 3 taps 658 -> 497 us, 5 taps 519 -> 490 us;
//   walk over tiled at 9 taps (level 3: 415 x 233 outputs, 4.6 source rows per destination row): 762 vs 813 us per 256;
//   rows + cols over tiled at 19 taps, 64 frames: 459 -> 244 us; 9 taps is still faster tiled (231 vs 254 us).
template <typename T>
PrepRoute prep_route(const T* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W, int H, int wk, int hk, int ksize)
{
    auto aligned = [&](int a) {
        return (row_stride % a) == 0 && (img_stride % a) == 0 && (reinterpret_cast<uintptr_t>(src) % a) == 0;
    };
    // the 4-pixel lanes' vector row loads: a dword (u8) / 8 bytes (16-bit) / 16 bytes (f32) at every 4th column
    const bool rows_va = aligned(4 * (int)sizeof(T));
    if (wk == W && hk == H) return ksize == 3 && (W & 3) == 0 && rows_va && W >= 8 ? ROUTE_SAME3_VEC : ROUTE_SAME;

    const double scale_x = inv_scale(wk, W), scale_y = inv_scale(hk, H);
    const bool downscale = scale_x >= 1.0 && scale_y >= 1.0;
    const int S = W / wk, CWL = decim_lane_cols(W);
    // 8-bit: a lane's CWL bytes are one load; 16-bit / f32: 8- / 16-byte aligned rows (4-pixel vector loads), and f32
    // takes 8-column lanes only while the blur halo fits in one (S = 2, 4)
    const bool decim_al = kU8<T> ? aligned(CWL) : rows_va && (CWL == 16 || S <= 4 || sizeof(T) == 2);
    const bool decim_ok = S >= 2 && W == S * wk && H == S * hk && (W % CWL) == 0 && W >= 64 && decim_al &&
                          ((S == 2 && ksize == 3) || (S == 4 && ksize == 9) || (S == 8 && ksize == 19)) && H > ksize;
    const bool walk_ok = downscale && scale_y < ksize && (ksize == 3 || ksize == 5 || ksize == 9);
    const bool direct_ok = downscale && (ksize == 3 || ksize == 5);
    if (decim_ok) return ROUTE_DECIM;
    if (walk_ok) return ROUTE_WALK;
    if (direct_ok) return ROUTE_DIRECT;
    if (downscale && ksize == 19) return ROUTE_ROWS_COLS;
    if (downscale && tiled_lds(scale_x, scale_y, ksize, sizeof(T)).bytes <= 60 * 1024) return ROUTE_TILED;
    return ROUTE_NAIVE;
}

template <typename T, bool FMA>
int prep_impl(nsof_ctx* ctx, int n_img, const T* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W, int H, int wk, int hk,
              const nsof_blur_taps& taps, float* out)
{
    nsof_prof_scope ps(ctx, NSOF_K_PREP);
    const double scale_x = inv_scale(wk, W), scale_y = inv_scale(hk, H);
    const dim3 block(256), per_pixel = nsof_pixel_grid(wk, hk, n_img);
    switch (prep_route(src, row_stride, img_stride, W, H, wk, hk, taps.ksize)) {
    case ROUTE_SAME3_VEC:
        hipLaunchKernelGGL((k_prep_same3_vec<false, T, FMA>), dim3((W / 4 + 63) / 64, (H + 4 * PREP0_ROWS - 1) / (4 * PREP0_ROWS), n_img),
                           block, 0, ctx->stream, src, row_stride, img_stride, W, H, taps.k[1], taps.k[2], out, nullptr);
        break;
    case ROUTE_SAME:
        hipLaunchKernelGGL((k_prep_same<false, T, FMA>), per_pixel, block, 0, ctx->stream, src, row_stride, img_stride, W, H, taps,
                           out, nullptr, -1);
        break;
    case ROUTE_DECIM: {
        const int S = W / wk, CWL = decim_lane_cols(W);
        // segments of output rows: multiples of the unroll count, ~16 source rows of warm-up amortised
        const int U = S == 2 ? 2 : 3;
        int seg_rows = S == 2 ? 32 : (S == 4 ? 24 : 15);
        seg_rows = (seg_rows + U - 1) / U * U;
        // few images (one call per camera frame): shorter segments so that the launch still has ~1000 waves
        const long waves_x = (W / CWL + 63) / 64;
        if (waves_x * ((hk + seg_rows - 1) / seg_rows) * n_img < 1024) {
            const long want_seg = (1024 + waves_x * n_img - 1) / (waves_x * n_img);
            seg_rows = std::min(seg_rows, (int)std::max<long>(U, (hk / want_seg) / U * U));
        }
        const int nseg = (hk + seg_rows - 1) / seg_rows;
        dim3 grid((unsigned)waves_x, (nseg + 3) / 4, n_img);
        // level k = 1, 2, 3 (S = 2^k with 3, 9, 19 taps) x 8- or 16-column lanes; no float 8-column walk at S = 8
        nsof_with_int<1, 3>(S == 2 ? 1 : (S == 4 ? 2 : 3), [&](auto k) {
            constexpr int SS = 1 << decltype(k)::value, KS = SS == 2 ? 3 : (SS == 4 ? 9 : 19);
            nsof_with_int<1, 2>(CWL / 8, [&](auto c) {
                constexpr int CW = 8 * decltype(c)::value;
                if constexpr (CW == 16 || SS < 8 || sizeof(T) <= 2)
                    hipLaunchKernelGGL((k_prep_decim<SS, KS, CW, T, FMA>), grid, block, 0, ctx->stream, src, row_stride, img_stride,
                                       W, H, wk, hk, seg_rows, taps, out);
            });
        });
        break;
    }
    case ROUTE_WALK: {
        // segments of destination rows: long enough that the KS + 1 rows of warm-up are a few per cent, short enough
        // that a small batch still has a few thousand waves
        const long waves_x = (wk + 63) / 64;
        const int seg_rows = segment_rows(32, 8, waves_x, hk, n_img, 2048, [](int rows) { return rows / 2; });
        const int nseg = (hk + seg_rows - 1) / seg_rows;
        dim3 grid((unsigned)waves_x, (nseg + 3) / 4, n_img);
        nsof_with_int<3, 9>(taps.ksize, [&](auto ks) {
            constexpr int KS = decltype(ks)::value;
            if constexpr (KS == 3 || KS == 5 || KS == 9)
                hipLaunchKernelGGL((k_prep_walk<KS, T, FMA>), grid, block, 0, ctx->stream, src, row_stride, img_stride, W, H, wk, hk,
                                   scale_x, scale_y, seg_rows, taps, out);
        });
        break;
    }
    case ROUTE_DIRECT:
        nsof_with_int<3, 5>(taps.ksize, [&](auto ks) {
            constexpr int KS = decltype(ks)::value;
            if constexpr (KS != 4)
                hipLaunchKernelGGL((k_prep_direct<KS, false, T, FMA>), per_pixel, block, 0, ctx->stream, src, row_stride, img_stride,
                                   W, H, wk, hk, scale_x, scale_y, taps, out, nullptr);
        });
        break;
    case ROUTE_ROWS_COLS: {
        int rc = ctx->tmp.reserve(ctx, (size_t)n_img * H * 2 * wk * sizeof(float));
        if (rc) return rc;
        float* HA = static_cast<float*>(ctx->tmp.p);
        dim3 ga((2 * wk + 63) / 64, (H + 4 * PREPA_ROWS - 1) / (4 * PREPA_ROWS), n_img);
        hipLaunchKernelGGL((k_prep_rows<19, T, FMA>), ga, block, 0, ctx->stream, src, row_stride, img_stride, W, H, wk, scale_x,
                           taps, HA);
        hipLaunchKernelGGL((k_prep_cols<19, FMA>), per_pixel, block, 0, ctx->stream, HA, W, H, wk, hk, scale_x, scale_y, taps, out);
        break;
    }
    case ROUTE_TILED: {
        int rc = launch_tiled<false, T, FMA>(ctx, tiled_grid(wk, hk, n_img), tiled_lds(scale_x, scale_y, taps.ksize, sizeof(T)), src,
                                             row_stride, img_stride, W, H, wk, hk, scale_x, scale_y, taps, out, nullptr);
        if (rc) return rc;
        break;
    }
    case ROUTE_NAIVE:
        hipLaunchKernelGGL((k_prep_naive<false, T, FMA>), per_pixel, block, 0, ctx->stream, src, row_stride, img_stride, W, H, wk,
                           hk, scale_x, scale_y, taps, out, nullptr);
        break;
    }
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// ---- work lists (shape-heterogeneous): one launch per level over a device table -----------------------------------
// T: the pixel type of every item's frames (the list's src_type).  The rule set is shorter than a uniform level's (no
// decimating walk, no row walk, no two-pass form): same-size levels as above, per item; 3 / 5 taps direct; then tiled
// within the LDS budget, else per pixel.  With 16-bit / float frames NSOF_HET_VEC0 means 8- / 16-byte aligned rows
// (k_prep_same3_vec's 4-pixel loads), the scalar k_prep_same takes the rest.  The LDS-tiled kernel's budget is 60 KB,
// and 78 KB for 16-bit frames: the 19-tap scale-8 level of large crops needs ~75 KB at 2 B/px (50 KB at 1), and two
// workgroups still fit the CU's 160 KB.
template <typename T, bool FMA>
int prep_het_impl(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, const nsof_het_item* h_items, bool level0,
                  const nsof_blur_taps& taps, float* I)
{
    nsof_prof_scope ps(ctx, NSOF_K_PREP);
    int max_wk = 0, max_hk = 0, n_vec = 0;
    double max_sx = 1, max_sy = 1;
    for (int i = 0; i < n_items; i++) {
        const nsof_het_item& it = h_items[i];
        max_wk = std::max(max_wk, it.wk);
        max_hk = std::max(max_hk, it.hk);
        n_vec += (it.flags & NSOF_HET_VEC0) ? 1 : 0;
        max_sx = std::max(max_sx, inv_scale(it.wk, it.W));
        max_sy = std::max(max_sy, inv_scale(it.hk, it.H));
    }
    const int nz = 2 * n_items;
    const dim3 block(256), per_pixel = nsof_pixel_grid(max_wk, max_hk, nz);
    const TiledLds lds = tiled_lds(max_sx, max_sy, taps.ksize, sizeof(T));
    if (level0) {   // same-size level: 3 taps; aligned items take the vector kernel, the others the generic one
        if (taps.ksize == 3 && n_vec > 0) {
            dim3 grid((max_wk / 4 + 63) / 64, (max_hk + 4 * PREP0_ROWS - 1) / (4 * PREP0_ROWS), nz);
            hipLaunchKernelGGL((k_prep_same3_vec<true, T, FMA>), grid, block, 0, ctx->stream, nullptr, 0, 0, 0, 0, taps.k[1],
                               taps.k[2], I, d_items);
        }
        if (taps.ksize != 3 || n_vec < n_items)
            hipLaunchKernelGGL((k_prep_same<true, T, FMA>), per_pixel, block, 0, ctx->stream, nullptr, 0, 0, 0, 0, taps, I, d_items,
                               taps.ksize == 3 ? 0 : -1);
    } else if (taps.ksize == 3 || taps.ksize == 5) {
        nsof_with_int<3, 5>(taps.ksize, [&](auto ks) {
            constexpr int KS = decltype(ks)::value;
            if constexpr (KS != 4)
                hipLaunchKernelGGL((k_prep_direct<KS, true, T, FMA>), per_pixel, block, 0, ctx->stream, nullptr, 0, 0, 0, 0, 0, 0, 1.,
                                   1., taps, I, d_items);
        });
    } else if (lds.bytes <= (sizeof(T) == 2 ? 78 : 60) * 1024) {
        int rc = launch_tiled<true, T, FMA>(ctx, tiled_grid(max_wk, max_hk, nz), lds, nullptr, 0, 0, 0, 0, 0, 0, 1., 1., taps, I,
                                            d_items);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL((k_prep_naive<true, T, FMA>), per_pixel, block, 0, ctx->stream, nullptr, 0, 0, 0, 0, 0, 0, 1., 1., taps, I,
                           d_items);
    }
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
}  // namespace

// f(nsof_px_tag<T>{}, std::bool_constant<FMA>{}) for a pixel type (nsof_src_type) and the context's arithmetic variant;
// false, f not called, for an unknown type.
namespace {
template <class Fn>
bool with_px_fma(const nsof_ctx* ctx, int src_type, Fn&& f)
{
    return nsof_with_src_type(src_type, [&](auto px_tag) { nsof_with_fma(ctx, [&](auto fma) { f(px_tag, fma); }); });
}
}  // namespace

// f32 frames take the three one-level launches (k_prep_decim<.., float>): at 768 threads per workgroup a wave has 168
// registers, and the float rows of the three walks side by side spilled (~400 registers' worth to scratch)
int nsof_launch_prep_decim3(nsof_ctx* ctx, int n_img, const void* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W, int H,
                            const nsof_blur_taps* taps, float* const* out, int src_type)
{
    int rc = NSOF_EUNSUPPORTED;
    with_px_fma(ctx, src_type, [&](auto px_tag, auto fma) {
        using T = typename decltype(px_tag)::type;
        if constexpr (kInt<T>)
            rc = prep_decim3_impl<T, decltype(fma)::value>(ctx, n_img, static_cast<const T*>(src), row_stride, img_stride, W, H, taps,
                                                           out);
    });
    return rc;
}

int nsof_launch_prep(nsof_ctx* ctx, int n_img, const void* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W, int H, int wk,
                     int hk, const nsof_blur_taps& taps, float* out, int src_type)
{
    int rc = NSOF_OK;
    const bool known = with_px_fma(ctx, src_type, [&](auto px_tag, auto fma) {
        using T = typename decltype(px_tag)::type;
        rc = prep_impl<T, decltype(fma)::value>(ctx, n_img, static_cast<const T*>(src), row_stride, img_stride, W, H, wk, hk, taps,
                                                out);
    });
    return known ? rc : nsof_set_error(ctx, NSOF_EINVAL, "unknown pixel type %d", src_type);
}

int nsof_launch_prep_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, const nsof_het_item* h_items, bool level0,
                         const nsof_blur_taps& taps, float* I, int src_type)
{
    int rc = NSOF_OK;
    const bool known = with_px_fma(ctx, src_type, [&](auto px_tag, auto fma) {
        using T = typename decltype(px_tag)::type;
        rc = prep_het_impl<T, decltype(fma)::value>(ctx, n_items, d_items, h_items, level0, taps, I);
    });
    return known ? rc : nsof_set_error(ctx, NSOF_EINVAL, "unknown pixel type %d", src_type);
}
