// Motion-segmentation head on the flow field (reference optical_flow_seg.py:253-357, 503-537):
//   mask = |flow| > SEG_TH ; 5 x (dilate, erode) with a 10x10 elliptical element ; 0/255.
//
// The masks are two-valued, so the head works on BIT-PACKED rows (one 32-bit word = 32 pixels):
//   k_mag_pack    flow [h][w][2] f32 -> bits, one wave ballot per 64 pixels.  HBM-bound: 8 B/px in, 1/8 B/px out.
//   k_u8_pack     any u8 image (non-zero = set) -> bits, for the dilate/erode mirror.
//   k_morph_bits  ALL passes of a dilate/erode chain in one launch.  A workgroup owns an output tile plus the halo
//                 the whole chain needs (passes * element reach), holds it in LDS, and per pass does
//                   H step: for every distinct row pattern of the element, OR of the funnel-shifted words
//                           (v_alignbit: one instruction per element column, 32 pixels at a time)
//                   V step: OR over the element rows of the matching H array
//                 erode = complement . dilate . complement with the same offsets (cv2 does not reflect the element).
//                 Pixels outside the image never take part (cv2's default border for morphology), which is the
//                 `inside` mask applied after every pass.  The bit image is 1/64 of the flow's size, so the halo
//                 re-reads are free and the head as a whole stays bound by the one read of the flow.
//   k_mag_pack_jobs / k_morph_jobs / k_mask_compose   the head over the boxes of a whole sequence: the bodies of the
//                 two kernels above (mag_pack_rows, morph_tile) applied per box (each box its own image) from
//                 host-built job lists, then one pass over every canvas pixel that takes the bit of the last box
//                 covering it (the paste order of the reference).
//   k_pa_partial / k_pa_final   pixel accuracy of a batch of masks against thresholded gray ground-truth frames,
//                 counted in integers.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "nsof_internal.h"

namespace {

constexpr int MAX_K = 32;         // element up to 32x32 (one 32-bit row pattern)
constexpr int MAX_DISTINCT = 16;
constexpr int TILE_H = 32;        // output rows per workgroup
constexpr int TILE_WORDS = 12;    // output words per workgroup (384 px)
constexpr int HALO_WORDS = 2;     // 64 px each side
constexpr int TW = TILE_WORDS + 2 * HALO_WORDS;   // 16 words per LDS row
constexpr int MORPH_THREADS = 1024;
constexpr int MAX_ROWS = 256;     // LDS rows per tile
static_assert(TW == 16, "index arithmetic below uses shifts by 4");

struct MorphElem {
    uint32_t extra[MAX_DISTINCT];    // pattern d = pattern base[d] | extra[d]   (bit j = element column j)
    int8_t base[MAX_DISTINCT];       // an earlier pattern that is a subset of d, or -1
    uint8_t row_pattern[MAX_K];      // pattern index of element row i, 0xff = empty row
    int n_patterns, kw, kh, ax, ay;
};

// One wave packs pixels k64 * 64 .. k64 * 64 + 63 of rows 8 by .. 8 by + 7: `mag > thresh` -> one ballot per row.
// The pointers are not __restrict__ here (the kernels' own parameters are): with the qualifier repeated on the inlined
// copy, k_mag_pack_jobs' loop recomputes its store addresses per row and the pack stage of a sequence measured 1-2 %
// slower; without it both kernels keep the loop, registers and instruction count they had with the body written out.
__device__ __forceinline__ void mag_pack_rows(const float* flow, ptrdiff_t fstride, int w, int h, double thresh,
                                              uint32_t* bits, int wp, int k64, int lane, int by)
{
    const int x = k64 * 64 + lane;
    const int y0 = by * 8;
    float2 v[8];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        v[r] = (x < w && y < h) ? *(const float2*)(flow + (ptrdiff_t)y * fstride + 2 * x) : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const double a = v[r].x, b = v[r].y;
        const bool set = x < w && y < h && sqrt(a * a + b * b) > thresh;   // cartToPolar on float64, then `mag > th`
        const unsigned long long m = __ballot(set);
        if (lane == 0 && y < h) *(unsigned long long*)(bits + (size_t)y * wp + 2 * k64) = m;
    }
}

__global__ __launch_bounds__(256) void k_mag_pack(const float* __restrict__ flow, ptrdiff_t fstride, int w, int h,
                                                  double thresh, uint32_t* __restrict__ bits, int wp)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k64 = blockIdx.x * 4 + wave;   // 64-pixel group of the row
    if (k64 * 2 >= wp) return;
    mag_pack_rows(flow, fstride, w, h, thresh, bits, wp, k64, lane, blockIdx.y);
}

__global__ __launch_bounds__(256) void k_u8_pack(const uint8_t* __restrict__ src, ptrdiff_t sstride, int w, int h,
                                                 uint32_t* __restrict__ bits, int wp)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k64 = blockIdx.x * 4 + wave;
    if (k64 * 2 >= wp) return;
    const int x = k64 * 64 + lane;
    const int y0 = blockIdx.y * 8;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const int y = y0 + r;
        const bool set = x < w && y < h && src[(ptrdiff_t)y * sstride + x] != 0;
        const unsigned long long m = __ballot(set);
        if (lane == 0 && y < h) *(unsigned long long*)(bits + (size_t)y * wp + 2 * k64) = m;
    }
}

// Bits of word gk of row gy that lie inside the image.
__device__ __forceinline__ uint32_t inside_bits(int gy, int gk, int w, int h)
{
    if (gy < 0 || gy >= h || gk < 0) return 0u;
    const int left = w - gk * 32;   // pixels of the row from this word on
    return left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : (1u << left) - 1u);
}

// Static recursion over the element description: every access to `el` has a compile-time index, so the whole
// description sits in scalar registers (indexing a kernel argument dynamically costs a scalar memory load per tap,
// which made the first version of this kernel 4x slower).
template <int D>
__device__ __forceinline__ void h_patterns(const MorphElem& el, uint32_t* H, int n, int i, uint32_t lo, uint32_t mid,
                                           uint32_t hi)
{
    if constexpr (D < MAX_DISTINCT) {
        if (D >= el.n_patterns) return;
        uint32_t acc = el.base[D] >= 0 ? H[el.base[D] * n + i] : 0u;
        for (uint32_t m = el.extra[D]; m; m &= m - 1) {   // constant trip count (unrolled) when FIXED10
            const int c = __builtin_ctz(m) - el.ax;    // out bit b takes in bit b + c
            acc |= c == 0 ? mid
                          : (c > 0 ? __builtin_amdgcn_alignbit(hi, mid, (unsigned)c)
                                   : __builtin_amdgcn_alignbit(mid, lo, (unsigned)(32 + c)));
        }
        H[D * n + i] = acc;
        h_patterns<D + 1>(el, H, n, i, lo, mid, hi);
    }
}

template <int E>
__device__ __forceinline__ uint32_t v_rows(const MorphElem& el, const uint32_t* H, int n, int r, int k, int rows)
{
    if constexpr (E < MAX_K) {
        if (E >= el.kh) return 0u;
        const int d = el.row_pattern[E];
        const int rr = r + E - el.ay;
        const uint32_t v = (d != 0xff && rr >= 0 && rr < rows) ? H[d * n + rr * TW + k] : 0u;
        return v | v_rows<E + 1>(el, H, n, r, k, rows);
    } else {
        return 0u;
    }
}

// The element of the reference (10x10 ellipse, centre anchor) as a compile-time constant: with it the H and V steps
// unroll into straight-line code (10 funnel shifts, 10 LDS reads per word); the run-time description costs scalar
// control flow per tap and is ~6x slower per pass.
constexpr MorphElem ellipse10()
{
    MorphElem e{};
    e.extra[0] = 0x020u; e.extra[1] = 0x1DCu; e.extra[2] = 0x202u; e.extra[3] = 0x001u;   // rows of 1, 7, 9, 10 pixels
    e.base[0] = -1; e.base[1] = 0; e.base[2] = 1; e.base[3] = 2;
    constexpr uint8_t rp[10] = {0, 1, 2, 3, 3, 3, 3, 3, 2, 1};
    for (int i = 0; i < 10; i++) e.row_pattern[i] = rp[i];
    e.n_patterns = 4; e.kw = 10; e.kh = 10; e.ax = 5; e.ay = 5;
    return e;
}

// One output tile (bx, by) of a chain launch; the whole workgroup runs it.  ops: bit p = 1 -> pass p is a dilate,
// 0 -> erode.  Output: out_u8 (0/255) when non-null, else out_bits.  FIXED10: ignore el_arg and use ellipse10().
template <bool FIXED10>
__device__ __forceinline__ void morph_tile(const uint32_t* __restrict__ in_bits, int wp, int w, int h,
                                           const MorphElem& el_arg, int n_pass, unsigned ops, int top, int rows,
                                           uint32_t* __restrict__ out_bits, uint8_t* __restrict__ out_u8,
                                           ptrdiff_t ostride, int bx, int by)
{
    constexpr MorphElem fixed = ellipse10();
    const MorphElem& el = FIXED10 ? fixed : el_arg;
    extern __shared__ uint32_t lds[];
    uint32_t* cur = lds;                       // [rows][TW]
    uint32_t* H = lds + (size_t)rows * TW;     // [n_patterns][rows][TW]
    const int tid = threadIdx.x;
    const int gk0 = bx * TILE_WORDS - HALO_WORDS;
    const int gy0 = by * TILE_H - top;
    const int n = rows * TW;
    const int k = tid & (TW - 1);              // 1024 % TW == 0: a thread keeps its word column
    const int gk = gk0 + k;

    for (int i = tid; i < n; i += MORPH_THREADS) {
        const int gy = gy0 + (i >> 4);
        cur[i] = (gy >= 0 && gy < h && gk >= 0 && gk < wp) ? in_bits[(size_t)gy * wp + gk] : 0u;
    }
    __syncthreads();

    for (int p = 0; p < n_pass; p++) {
        const bool dil = (ops >> p) & 1u;
        // H step: per distinct row pattern, OR of the funnel-shifted words (one v_alignbit per element column)
        for (int i = tid; i < n; i += MORPH_THREADS) {
            const int gy = gy0 + (i >> 4);
            uint32_t lo = k > 0 ? cur[i - 1] : 0u, mid = cur[i], hi = k + 1 < TW ? cur[i + 1] : 0u;
            if (!dil) {   // complement inside the image; outside stays 0 (= "does not take part" in a minimum)
                lo = k > 0 ? ~lo & inside_bits(gy, gk - 1, w, h) : 0u;
                mid = ~mid & inside_bits(gy, gk, w, h);
                hi = k + 1 < TW ? ~hi & inside_bits(gy, gk + 1, w, h) : 0u;
            }
            h_patterns<0>(el, H, n, i, lo, mid, hi);
        }
        __syncthreads();
        // V step: OR over the element rows of the matching H array
        for (int i = tid; i < n; i += MORPH_THREADS) {
            const int r = i >> 4;
            const uint32_t acc = v_rows<0>(el, H, n, r, k, rows);
            cur[i] = (dil ? acc : ~acc) & inside_bits(gy0 + r, gk, w, h);
        }
        __syncthreads();
    }

    // write the tile's own rows/words
    if (out_u8) {
        for (int i = tid; i < TILE_H * TILE_WORDS * 8; i += MORPH_THREADS) {   // 4 pixels per item
            const int r = i / (TILE_WORDS * 8), q = i - r * (TILE_WORDS * 8);
            const int gy = by * TILE_H + r, gx = bx * TILE_WORDS * 32 + q * 4;
            if (gy >= h || gx >= w) continue;
            const uint32_t word = cur[(r + top) * TW + HALO_WORDS + (q >> 3)];
            const uint32_t nib = (word >> ((q & 7) * 4)) & 0xfu;
            uint8_t* o = out_u8 + (ptrdiff_t)gy * ostride + gx;
            if (gx + 4 <= w && (((uintptr_t)o) & 3) == 0) {
                *(uint32_t*)o = ((nib & 1u) ? 0xffu : 0u) | ((nib & 2u) ? 0xff00u : 0u) | ((nib & 4u) ? 0xff0000u : 0u) |
                                ((nib & 8u) ? 0xff000000u : 0u);
            } else {
                for (int b = 0; b < 4 && gx + b < w; b++) o[b] = (nib >> b) & 1u ? 255 : 0;
            }
        }
    } else {
        for (int i = tid; i < TILE_H * TILE_WORDS; i += MORPH_THREADS) {
            const int r = i / TILE_WORDS, kk = i - r * TILE_WORDS;
            const int gy = by * TILE_H + r, gk = bx * TILE_WORDS + kk;
            if (gy < h && gk < wp) out_bits[(size_t)gy * wp + gk] = cur[(r + top) * TW + HALO_WORDS + kk];
        }
    }
}

template <bool FIXED10>
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_bits(const uint32_t* __restrict__ in_bits, int wp, int w,
                                                              int h, const MorphElem el_arg, int n_pass, unsigned ops,
                                                              int top, int rows, uint32_t* __restrict__ out_bits,
                                                              uint8_t* __restrict__ out_u8, ptrdiff_t ostride)
{
    morph_tile<FIXED10>(in_bits, wp, w, h, el_arg, n_pass, ops, top, rows, out_bits, out_u8, ostride, blockIdx.x,
                        blockIdx.y);
}

// ---- the head over the boxes of a whole sequence (nsof_motion_mask_sequence_dev) --------------------------------
// Every non-empty box is an image of its own (cv2 sees the crop: its edges are image borders), with two bit images
// in the workspace.  The host lists the boxes and one job per workgroup of each stage, so the grids are exact.
struct SegBox {
    unsigned long long off;   // word offset of the box's bit images in the workspace: A at off, B at off + wp * h
    int pair, x0, y0, w, h, wp;
};
struct SegJob {
    int box;
    int tile;                 // pack: the 8-row group; morph: ty * tiles_x + tx
};

// Pack: one workgroup per (box, 8-row group); its 4 waves walk the row's 64-pixel groups.  Pair p's flow canvas is
// [H][W][2] at flows + p * H * W * 2; the crop keeps the canvas row stride.
__global__ __launch_bounds__(256) void k_mag_pack_jobs(const SegJob* __restrict__ jobs, const SegBox* __restrict__ boxes,
                                                       const float* __restrict__ flows, int W, int H, double thresh,
                                                       uint32_t* __restrict__ ws)
{
    const SegJob j = jobs[blockIdx.x];
    const SegBox box = boxes[j.box];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* flow = flows + (((size_t)box.pair * H + box.y0) * W + box.x0) * 2;
    for (int k64 = wave; k64 * 2 < box.wp; k64 += 4)
        mag_pack_rows(flow, 2 * (ptrdiff_t)W, box.w, box.h, thresh, ws + box.off, box.wp, k64, lane, j.tile);
}

// Morph: one workgroup per (box, tile), the tile walk of k_morph_bits on the box's own image.  src_b: read B, write A.
template <bool FIXED10>
__global__ __launch_bounds__(MORPH_THREADS) void k_morph_jobs(const SegJob* __restrict__ jobs,
                                                              const SegBox* __restrict__ boxes, uint32_t* __restrict__ ws,
                                                              int src_b, const MorphElem el_arg, int n_pass,
                                                              unsigned ops, int top, int rows)
{
    const SegJob j = jobs[blockIdx.x];
    const SegBox box = boxes[j.box];
    const int tiles_x = (box.wp + TILE_WORDS - 1) / TILE_WORDS;
    const int ty = j.tile / tiles_x, tx = j.tile - ty * tiles_x;
    const size_t img = (size_t)box.wp * box.h;
    morph_tile<FIXED10>(ws + box.off + (src_b ? img : 0), box.wp, box.w, box.h, el_arg, n_pass, ops, top, rows,
                        ws + box.off + (src_b ? 0 : img), nullptr, 0, tx, ty);
}

// Compose: 4 canvas pixels per thread (256 x 4 per workgroup), blockIdx.z = pair.  A pixel takes the bit of the LAST
// of its pair's boxes that covers it (the paste order of optical_flow_seg.py), 0 when none does; the scan walks the
// pair's boxes from the end and stops once all 4 pixels are decided, so it has no cap on the box count.
__global__ __launch_bounds__(256) void k_mask_compose(const SegBox* __restrict__ boxes, const int* __restrict__ first,
                                                      const uint32_t* __restrict__ ws, int final_b, int w, int h,
                                                      uint8_t* __restrict__ masks)
{
    const int x = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4, y = blockIdx.y * 4 + (threadIdx.x >> 6), k = blockIdx.z;
    if (x >= w || y >= h) return;
    const int n = min(4, w - x);
    unsigned pending = (1u << n) - 1u, v = 0;
    for (int i = first[k + 1] - 1; i >= first[k] && pending; i--) {
        const SegBox b = boxes[i];
        const int ry = y - b.y0;
        if (ry < 0 || ry >= b.h) continue;
        const uint32_t* row = ws + b.off + (final_b ? (size_t)b.wp * b.h : 0) + (size_t)ry * b.wp;
        for (int p = 0; p < n; p++) {
            const int rx = x + p - b.x0;
            if (!((pending >> p) & 1u) || rx < 0 || rx >= b.w) continue;
            pending &= ~(1u << p);
            if ((row[rx >> 5] >> (rx & 31)) & 1u) v |= 0xffu << (8 * p);
        }
    }
    uint8_t* o = masks + ((size_t)k * h + y) * w + x;
    if (n == 4 && (((uintptr_t)o) & 3) == 0) {
        *(uint32_t*)o = v;
    } else {
        for (int p = 0; p < n; p++) o[p] = (uint8_t)(v >> (8 * p));
    }
}

// ---- pixel accuracy of a batch (nsof_pixel_accuracy_u8_batch_dev) ------------------------------------------------
constexpr int PA_ROWS = 8;   // rows per workgroup of the partial counts

// Equal pixels of mask rows by*8 .. by*8+7 against (gray(gt) > 127 ? 255 : 0), blockIdx.z = item; integer partials.
__global__ __launch_bounds__(256) void k_pa_partial(const uint8_t* __restrict__ masks, const uint8_t* __restrict__ gt,
                                                    ptrdiff_t gt_row_stride, ptrdiff_t gt_frame_stride, int w, int h,
                                                    unsigned* __restrict__ partial)
{
    __shared__ unsigned red[4];
    const int k = blockIdx.z, y0 = blockIdx.x * PA_ROWS;
    const int rows = min(PA_ROWS, h - y0);
    const uint8_t* m = masks + ((size_t)k * h + y0) * w;
    const uint8_t* g = gt + (ptrdiff_t)k * gt_frame_stride + (ptrdiff_t)y0 * gt_row_stride;
    unsigned cnt = 0;
    for (int r = 0; r < rows; r++)
        for (int x = threadIdx.x; x < w; x += 256) {
            const uint8_t* px = g + (ptrdiff_t)r * gt_row_stride + 3 * (ptrdiff_t)x;
            const unsigned t = nsof_gray_px(px[0], px[1], px[2], 3735, 19235, 9798) > 127 ? 255u : 0u;   // BGR2GRAY
            cnt += m[(size_t)r * w + x] == t;
        }
    for (int d = 32; d > 0; d >>= 1) cnt += __shfl_down(cnt, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)k * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One workgroup per item (blockIdx.x): the sum of its n partials -> count / (w * h) * 100, as calculate_pixel_accuracy.
__global__ __launch_bounds__(256) void k_pa_final(const unsigned* __restrict__ partial, int n, double pixels,
                                                  double* __restrict__ out)
{
    __shared__ unsigned long long red[4];
    partial += (size_t)blockIdx.x * n;
    unsigned long long acc = 0;
    for (int i = threadIdx.x; i < n; i += 256) acc += partial[i];
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (double)(red[0] + red[1] + red[2] + red[3]) / pixels * 100.0;
}

int build_elem(nsof_ctx* ctx, const uint8_t* elem, int kw, int kh, int ax, int ay, MorphElem* out)
{
    if (kw < 1 || kh < 1 || kw > MAX_K || kh > MAX_K)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "structuring element %dx%d: sizes 1..%d supported", kw, kh, MAX_K);
    if (ax < 0) ax = kw / 2;
    if (ay < 0) ay = kh / 2;
    if (ax >= kw || ay >= kh) return nsof_set_error(ctx, NSOF_EINVAL, "anchor (%d,%d) outside the element", ax, ay);
    MorphElem e{};
    e.kw = kw; e.kh = kh; e.ax = ax; e.ay = ay;
    uint32_t rowpat[MAX_K], pats[MAX_DISTINCT];
    int np = 0;
    for (int i = 0; i < kh; i++) {
        uint32_t pat = 0;
        for (int j = 0; j < kw; j++)
            if (elem[i * kw + j]) pat |= 1u << j;
        rowpat[i] = pat;
        if (!pat) continue;
        int d = 0;
        while (d < np && pats[d] != pat) d++;
        if (d == np) {
            if (np == MAX_DISTINCT)
                return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "more than %d distinct element rows", MAX_DISTINCT);
            pats[np++] = pat;
        }
    }
    // order by population so that a pattern can build on an earlier subset (the rows of an ellipse nest)
    for (int a = 1; a < np; a++)
        for (int b = a; b > 0 && __builtin_popcount(pats[b]) < __builtin_popcount(pats[b - 1]); b--) {
            uint32_t t = pats[b]; pats[b] = pats[b - 1]; pats[b - 1] = t;
        }
    for (int d = 0; d < np; d++) {
        int best = -1;
        for (int c = 0; c < d; c++)
            if ((pats[c] & ~pats[d]) == 0 && (best < 0 || __builtin_popcount(pats[c]) > __builtin_popcount(pats[best])))
                best = c;
        e.base[d] = (int8_t)best;
        e.extra[d] = best >= 0 ? pats[d] & ~pats[best] : pats[d];
    }
    e.n_patterns = np;
    for (int i = 0; i < kh; i++) {
        int d = 0xff;
        if (rowpat[i])
            for (d = 0; pats[d] != rowpat[i]; d++) {}
        e.row_pattern[i] = (uint8_t)d;
    }
    *out = e;
    return NSOF_OK;
}

inline int words_per_row(int w) { return 2 * ((w + 63) / 64); }

// Passes the next launch of a chain takes (at most `left`), its LDS tile rows and bytes: the halo must hold the
// chunk's horizontal reach and the tile ((1 + patterns) arrays of rows x TW words) must fit the LDS.  Returns the pass
// count, or an nsof_status (< 0) when not even one pass fits.
int plan_chunk(nsof_ctx* ctx, const MorphElem& el, int left, int* rows_out, size_t* smem_out)
{
    const int reach_x = el.ax > el.kw - 1 - el.ax ? el.ax : el.kw - 1 - el.ax;
    const int up = el.ay, down = el.kh - 1 - el.ay;
    int chunk = left;
    if (reach_x > 0 && chunk > (HALO_WORDS * 32) / reach_x) chunk = (HALO_WORDS * 32) / reach_x;
    size_t smem;
    int rows;
    for (;; chunk--) {   // LDS budget: (1 + patterns) arrays of rows x TW words
        rows = TILE_H + chunk * (up + down);
        smem = (size_t)(1 + (el.n_patterns ? el.n_patterns : 1)) * rows * TW * 4;
        if ((smem <= 144 * 1024 && rows <= MAX_ROWS) || chunk <= 1) break;
    }
    if (chunk < 1 || smem > 160 * 1024 || rows > MAX_ROWS)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "structuring element too tall for the LDS tile");
    *rows_out = rows;
    *smem_out = smem;
    return chunk;
}

// The one place a chain is run: `ops` (n_pass passes) of element `el`, split into launches by plan_chunk, ping-pong
// between bit images A and B starting from A.  kern_fixed / kern_any are the FIXED10 / run-time-element arms of the
// kernel; launch(kern, smem, src_b, last, chunk, ops, top, rows) starts one chunk that reads B when src_b, else A, and
// writes the other.  Returns which image holds the result (0 = A, 1 = B), or an nsof_status (< 0).
template <class Kern, class Launch>
int run_chain(nsof_ctx* ctx, const MorphElem& el, int n_pass, unsigned ops, Kern kern_fixed, Kern kern_any,
              Launch launch)
{
    constexpr MorphElem e10 = ellipse10();
    const Kern kern = memcmp(&el, &e10, sizeof(MorphElem)) == 0 ? kern_fixed : kern_any;
    int src_b = 0;
    for (int done = 0; done < n_pass; src_b ^= 1) {
        size_t smem;
        int rows;
        const int chunk = plan_chunk(ctx, el, n_pass - done, &rows, &smem);
        if (chunk < 0) return chunk;
        if (smem > 64 * 1024)
            NSOF_HIP(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        {
            nsof_prof_scope ps(ctx, NSOF_K_MORPH);
            launch(kern, smem, src_b, done + chunk >= n_pass, chunk, ops >> done, chunk * el.ay, rows);
        }
        NSOF_HIP(ctx, hipGetLastError());
        done += chunk;
    }
    return src_b;
}

// The chain on one w x h image as a grid of tiles: a holds the input, b is the second bit image; the last chunk writes
// out_u8 when it is non-null.
int run_chain_image(nsof_ctx* ctx, uint32_t* a, uint32_t* b, int w, int h, const MorphElem& el, int n_pass,
                    unsigned ops, uint8_t* out_u8, ptrdiff_t ostride)
{
    const int wp = words_per_row(w);
    const dim3 grid((wp + TILE_WORDS - 1) / TILE_WORDS, (h + TILE_H - 1) / TILE_H);
    uint32_t* const img[2] = {a, b};
    return run_chain(ctx, el, n_pass, ops, k_morph_bits<true>, k_morph_bits<false>,
                     [&](auto kern, size_t smem, int src_b, bool last, int chunk, unsigned chunk_ops, int top, int rows) {
                         uint8_t* const u8 = last ? out_u8 : nullptr;
                         hipLaunchKernelGGL(kern, grid, dim3(MORPH_THREADS), smem, ctx->stream, img[src_b], wp, w, h, el,
                                            chunk, chunk_ops, top, rows, u8 ? nullptr : img[src_b ^ 1], u8, ostride);
                     });
}

// The chain of the motion head: `iterations` x (dilate, erode) with the ksize x ksize ellipse; with no iterations a
// single identity pass (1x1 element).  Validates ksize (iterations are the caller's).
int mask_chain(nsof_ctx* ctx, int ksize, int iterations, MorphElem* el, int* n_pass, unsigned* ops)
{
    if (ksize < 1 || ksize > MAX_K) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "ksize 1..%d supported", MAX_K);
    if (iterations == 0) ksize = 1;   // the 1x1 ellipse is the one set pixel
    uint8_t elem[MAX_K * MAX_K];
    nsof_structuring_element(NSOF_MORPH_ELLIPSE, ksize, ksize, elem);
    *ops = 1u;
    for (int k = 1; k < iterations; k++) *ops |= 1u << (2 * k);   // even passes dilate, odd passes erode
    *n_pass = iterations ? 2 * iterations : 1;
    return build_elem(ctx, elem, ksize, ksize, -1, -1, el);
}

inline dim3 pack_grid(int wp, int h) { return dim3((wp / 2 + 3) / 4, (h + 7) / 8); }   // 4 waves x 64 px, 8 rows

int reserve_bits(nsof_ctx* ctx, int w, int h, uint32_t** a, uint32_t** b)
{
    const size_t one = ((size_t)words_per_row(w) * h * 4 + 255) & ~(size_t)255;
    int rc = ctx->tmp.reserve(ctx, 2 * one);
    if (rc) return rc;
    *a = (uint32_t*)ctx->tmp.p;
    *b = (uint32_t*)((char*)ctx->tmp.p + one);
    return NSOF_OK;
}

}  // namespace

// cv::getStructuringElement for the shapes the reference uses (ellipse) and the trivial ones.  Host arithmetic only.
extern "C" int nsof_structuring_element(int shape, int kw, int kh, uint8_t* out)
{
    if (!out || kw < 1 || kh < 1 || shape < 0 || shape > 2) return NSOF_EINVAL;
    const int r = kh / 2, c = kw / 2;
    const double inv_r2 = r ? 1.0 / ((double)r * r) : 0.0;
    for (int i = 0; i < kh; i++) {
        int j1 = 0, j2 = 0;
        if (shape == NSOF_MORPH_RECT || (shape == NSOF_MORPH_CROSS && i == r)) {
            j2 = kw;
        } else if (shape == NSOF_MORPH_CROSS) {
            j1 = c;
            j2 = c + 1;
        } else {
            const int dy = i - r;
            if (abs(dy) <= r) {
                const int dx = (int)lrint(c * sqrt((r * r - dy * dy) * inv_r2));
                j1 = c - dx > 0 ? c - dx : 0;
                j2 = c + dx + 1 < kw ? c + dx + 1 : kw;
            }
        }
        for (int j = 0; j < kw; j++) out[i * kw + j] = (uint8_t)(j >= j1 && j < j2);
    }
    return NSOF_OK;
}

extern "C" int nsof_morph_binary_u8_dev(nsof_ctx* ctx, int op, const uint8_t* d_src, ptrdiff_t src_stride, int width,
                                        int height, const uint8_t* elem, int kw, int kh, int ax, int ay,
                                        int iterations, uint8_t* d_dst, ptrdiff_t dst_stride)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_src || !d_dst || !elem) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
    if (op != NSOF_MORPH_ERODE && op != NSOF_MORPH_DILATE) return nsof_set_error(ctx, NSOF_EINVAL, "op must be 0 or 1");
    if (width < 1 || height < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "empty image");
    if (iterations < 1 || iterations > 32) return nsof_set_error(ctx, NSOF_EINVAL, "iterations must be 1..32");
    if (src_stride < width || dst_stride < width) return nsof_set_error(ctx, NSOF_EINVAL, "stride < width");
    MorphElem el;
    int rc = build_elem(ctx, elem, kw, kh, ax, ay, &el);
    if (rc) return rc;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *a, *b;
    if ((rc = reserve_bits(ctx, width, height, &a, &b))) return rc;
    const int wp = words_per_row(width);
    {
        nsof_prof_scope ps(ctx, NSOF_K_SEGMENT);
        hipLaunchKernelGGL(k_u8_pack, pack_grid(wp, height), dim3(256), 0, ctx->stream, d_src, src_stride, width,
                           height, a, wp);
    }
    NSOF_HIP(ctx, hipGetLastError());
    rc = run_chain_image(ctx, a, b, width, height, el, iterations, op == NSOF_MORPH_DILATE ? 0xffffffffu : 0u, d_dst,
                         dst_stride);
    return rc < 0 ? rc : NSOF_OK;
}

extern "C" int nsof_motion_mask_dev(nsof_ctx* ctx, const float* d_flow, ptrdiff_t flow_stride_floats, int width,
                                    int height, double thresh, int ksize, int iterations, uint8_t* d_mask,
                                    ptrdiff_t mask_stride)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_flow || !d_mask) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
    if (width < 1 || height < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "empty flow field");
    if (iterations < 0 || iterations > 16) return nsof_set_error(ctx, NSOF_EINVAL, "iterations must be 0..16");
    if (flow_stride_floats < 2 * (ptrdiff_t)width || (flow_stride_floats & 1) || mask_stride < width)
        return nsof_set_error(ctx, NSOF_EINVAL, "bad stride");
    MorphElem el;
    int n_pass;
    unsigned ops;
    int rc = mask_chain(ctx, ksize, iterations, &el, &n_pass, &ops);
    if (rc) return rc;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t *a, *b;
    if ((rc = reserve_bits(ctx, width, height, &a, &b))) return rc;
    const int wp = words_per_row(width);
    {
        nsof_prof_scope ps(ctx, NSOF_K_SEGMENT);
        hipLaunchKernelGGL(k_mag_pack, pack_grid(wp, height), dim3(256), 0, ctx->stream, d_flow, flow_stride_floats,
                           width, height, thresh, a, wp);
    }
    NSOF_HIP(ctx, hipGetLastError());
    rc = run_chain_image(ctx, a, b, width, height, el, n_pass, ops, d_mask, mask_stride);
    return rc < 0 ? rc : NSOF_OK;
}

extern "C" int nsof_motion_mask(nsof_ctx* ctx, const float* flow, ptrdiff_t flow_stride_bytes, int width, int height,
                                double thresh, int ksize, int iterations, uint8_t* mask, ptrdiff_t mask_stride)
{
    if (!ctx) return NSOF_EINVAL;
    if (!flow || !mask) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
    if (width < 1 || height < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "empty flow field");
    if (flow_stride_bytes < (ptrdiff_t)width * 8 || mask_stride < width)
        return nsof_set_error(ctx, NSOF_EINVAL, "bad stride");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n0 = (size_t)width * height;
    const size_t szF = (n0 * 8 + 255) & ~(size_t)255, szM = (n0 + 255) & ~(size_t)255;
    int rc;
    if ((rc = ctx->stage.reserve(ctx, szF + szM))) return rc;
    if ((rc = ctx->hstage.reserve(ctx, szF + szM))) return rc;
    float* hF = (float*)ctx->hstage.p;
    uint8_t* hM = (uint8_t*)ctx->hstage.p + szF;
    float* dF = (float*)ctx->stage.p;
    uint8_t* dM = (uint8_t*)ctx->stage.p + szF;
    const bool in_dense = flow_stride_bytes == (ptrdiff_t)width * 8, out_dense = mask_stride == width;
    if (!in_dense)
        for (int y = 0; y < height; y++)
            memcpy(hF + (size_t)y * width * 2, (const char*)flow + (ptrdiff_t)y * flow_stride_bytes, (size_t)width * 8);
    NSOF_HIP(ctx, hipMemcpyAsync(dF, in_dense ? flow : hF, n0 * 8, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = nsof_motion_mask_dev(ctx, dF, 2 * (ptrdiff_t)width, width, height, thresh, ksize, iterations, dM, width)))
        return rc;
    NSOF_HIP(ctx, hipMemcpyAsync(out_dense ? mask : hM, dM, n0, hipMemcpyDeviceToHost, ctx->stream));
    if (int rcs = nsof_stream_sync_checked(ctx)) return rcs;   // incl. a lost hand-over of the exact-order flow kernels
    if (!out_dense)
        for (int y = 0; y < height; y++) memcpy(mask + (ptrdiff_t)y * mask_stride, hM + (size_t)y * width, (size_t)width);
    return NSOF_OK;
}

extern "C" int nsof_motion_mask_sequence_dev(nsof_ctx* ctx, int n_pairs, const float* d_flows, int width, int height,
                                             const int32_t* box_counts, const int32_t* boxes, double thresh, int ksize,
                                             int iterations, uint8_t* d_masks)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_flows || !d_masks) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
    if (n_pairs < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "mask_sequence: n_pairs %d < 1", n_pairs);
    if (n_pairs > 65535) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "mask_sequence: more than 65535 pairs");
    if (width < 1 || height < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "empty flow field");
    if (iterations < 0 || iterations > 16) return nsof_set_error(ctx, NSOF_EINVAL, "iterations must be 0..16");
    if (reinterpret_cast<uintptr_t>(d_flows) & 7) return nsof_set_error(ctx, NSOF_EINVAL, "flows must be 8-byte aligned");
    MorphElem el;
    int n_pass;
    unsigned ops;
    int rc = mask_chain(ctx, ksize, iterations, &el, &n_pass, &ops);
    if (rc) return rc;
    // the box list (empty boxes dropped, paste order kept), the first box of every pair, the two job lists
    std::vector<SegBox> bx;
    std::vector<int> first(n_pairs + 1);
    size_t words = 0;
    for (int k = 0, i = 0; k < n_pairs; k++) {
        first[k] = (int)bx.size();
        const int cnt = box_counts ? box_counts[k] : 1;
        if (cnt < 0) return nsof_set_error(ctx, NSOF_EINVAL, "mask_sequence: box count %d of pair %d", cnt, k);
        if (cnt > 0 && box_counts && !boxes) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
        for (int c = 0; c < cnt; c++, i += box_counts ? 1 : 0) {
            const int32_t* r = box_counts ? boxes + 4 * (size_t)i : nullptr;
            const int x0 = r ? r[0] : 0, y0 = r ? r[1] : 0, x1 = r ? r[2] : width, y1 = r ? r[3] : height;
            if (x1 <= x0 || y1 <= y0) continue;
            if (x0 < 0 || y0 < 0 || x1 > width || y1 > height)
                return nsof_set_error(ctx, NSOF_EINVAL, "mask_sequence: box (%d,%d,%d,%d) of pair %d leaves the %dx%d frame",
                                      x0, y0, x1, y1, k, width, height);
            SegBox b;
            b.pair = k; b.x0 = x0; b.y0 = y0; b.w = x1 - x0; b.h = y1 - y0; b.wp = words_per_row(b.w);
            b.off = words;
            words += (2 * (size_t)b.wp * b.h + 63) & ~(size_t)63;   // A and B, 256-byte aligned
            bx.push_back(b);
        }
    }
    first[n_pairs] = (int)bx.size();
    if (bx.size() > (size_t)INT32_MAX) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "mask_sequence: too many boxes");
    std::vector<SegJob> pack, morph;
    for (size_t i = 0; i < bx.size(); i++) {
        for (int t = 0; t < (bx[i].h + 7) / 8; t++) pack.push_back(SegJob{(int)i, t});
        const int tiles = (bx[i].wp + TILE_WORDS - 1) / TILE_WORDS * ((bx[i].h + TILE_H - 1) / TILE_H);
        for (int t = 0; t < tiles; t++) morph.push_back(SegJob{(int)i, t});
    }
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    // one table: boxes | first | pack jobs | morph jobs, through the pinned copy (rewritten only after its last upload)
    auto up16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t o_first = up16(bx.size() * sizeof(SegBox)), o_pack = o_first + up16(first.size() * sizeof(int));
    const size_t o_morph = o_pack + up16(pack.size() * sizeof(SegJob));
    const size_t bytes = o_morph + morph.size() * sizeof(SegJob);
    if ((rc = ctx->seg.stage(ctx, bytes, (bytes + bytes / 2 + 4095) & ~(size_t)4095))) return rc;
    if ((rc = ctx->tmp.reserve(ctx, words * 4 > 256 ? words * 4 : 256))) return rc;
    char* h = (char*)ctx->seg.h.p;
    memcpy(h, bx.data(), bx.size() * sizeof(SegBox));
    memcpy(h + o_first, first.data(), first.size() * sizeof(int));
    memcpy(h + o_pack, pack.data(), pack.size() * sizeof(SegJob));
    memcpy(h + o_morph, morph.data(), morph.size() * sizeof(SegJob));
    const char* d = (const char*)ctx->seg.upload(ctx, bytes);
    if (!d) return NSOF_EDEVICE;
    const SegBox* d_boxes = (const SegBox*)d;
    const SegJob* d_pack = (const SegJob*)(d + o_pack);
    const SegJob* d_morph = (const SegJob*)(d + o_morph);
    uint32_t* ws = (uint32_t*)ctx->tmp.p;
    constexpr size_t MAX_JOBS = 1u << 20;   // workgroups per launch (grid x threads stays far below 2^32)
    int final_b = 0;
    if (!bx.empty()) {
        {
            nsof_prof_scope ps(ctx, NSOF_K_SEGMENT);
            for (size_t i = 0; i < pack.size(); i += MAX_JOBS)
                hipLaunchKernelGGL(k_mag_pack_jobs, dim3((unsigned)std::min(MAX_JOBS, pack.size() - i)), dim3(256), 0,
                                   ctx->stream, d_pack + i, d_boxes, d_flows, width, height, thresh, ws);
        }
        NSOF_HIP(ctx, hipGetLastError());
        final_b = run_chain(ctx, el, n_pass, ops, k_morph_jobs<true>, k_morph_jobs<false>,
                            [&](auto kern, size_t smem, int src_b, bool, int chunk, unsigned chunk_ops, int top, int rows) {
                                for (size_t i = 0; i < morph.size(); i += MAX_JOBS)
                                    hipLaunchKernelGGL(kern, dim3((unsigned)std::min(MAX_JOBS, morph.size() - i)),
                                                       dim3(MORPH_THREADS), smem, ctx->stream, d_morph + i, d_boxes, ws,
                                                       src_b, el, chunk, chunk_ops, top, rows);
                            });
        if (final_b < 0) return final_b;
    }
    {
        nsof_prof_scope ps(ctx, NSOF_K_SEGMENT);
        hipLaunchKernelGGL(k_mask_compose, dim3((width + 255) / 256, (height + 3) / 4, n_pairs), dim3(256), 0, ctx->stream,
                           d_boxes, (const int*)(d + o_first), ws, final_b, width, height, d_masks);
    }
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_pixel_accuracy_u8_batch_dev(nsof_ctx* ctx, int n, const uint8_t* d_masks, const uint8_t* d_gt,
                                                ptrdiff_t gt_row_stride, ptrdiff_t gt_frame_stride, int width, int height,
                                                double* d_out)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_masks || !d_gt || !d_out) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
    if (n < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "pixel_accuracy: n %d < 1", n);
    if (n > 65535) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "pixel_accuracy: more than 65535 items");
    if (width < 1 || height < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "empty image");
    if (gt_row_stride < 3 * (ptrdiff_t)width || (n > 1 && gt_frame_stride < gt_row_stride * height))
        return nsof_set_error(ctx, NSOF_EINVAL, "pixel_accuracy: gt stride");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const int nblk = (height + PA_ROWS - 1) / PA_ROWS;
    int rc = ctx->tmp.reserve(ctx, (size_t)n * nblk * sizeof(unsigned));
    if (rc) return rc;
    unsigned* partial = (unsigned*)ctx->tmp.p;
    {
        nsof_prof_scope ps(ctx, NSOF_K_SEGMENT);
        hipLaunchKernelGGL(k_pa_partial, dim3(nblk, 1, n), dim3(256), 0, ctx->stream, d_masks, d_gt, gt_row_stride,
                           gt_frame_stride, width, height, partial);
    }
    hipLaunchKernelGGL(k_pa_final, dim3(n), dim3(256), 0, ctx->stream, partial, nblk,
                       (double)((long long)width * height), d_out);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
