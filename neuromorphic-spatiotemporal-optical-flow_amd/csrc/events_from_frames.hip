// Event streams from frame sequences (nsof_events_from_frames_count_dev / _emit_dev): a per-pixel
// level-crossing event generator, the contrast-threshold model of an event camera, all in integers.  A pixel keeps a
// reference level r; a frame of level b = lut[F] that lies c_on or more above r gives (b - r) / c_on ON events at the
// levels r + j * c_on, one c_off or more below gives (r - b) / c_off OFF events at r - j * c_off, and r follows by as
// many thresholds.  The output size depends on the data, so there are two passes over the frames:
//
//   k_ef_count   a thread owns a pixel (workgroups own 256 consecutive pixels in y * W + x order) and walks the frames in
//                order with r in a register, EF_BATCH frames at a time (their loads are issued before the first is used);
//                per frame and polarity the wave adds its lanes' counts (a DPP prefix sum in 32 bits while every lane's
//                count is below 2^24, else a 64-bit butterfly) and, once per batch, the workgroup's first 2 * EF_BATCH
//                threads add the four waves' sums into counts[frame][polarity][workgroup].
//   k_ef_scan    an exclusive scan of every row of that table in place (one workgroup per row, 256 entries at a time)
//                and the rows' sums; a second launch scans the 2 n sums: the bases of the (frame, polarity) rows and the total.
//   k_ef_emit    the same walk; per batch the waves take an inclusive prefix (DPP) of the counts of each frame and polarity,
//                the four waves' sums go through LDS, and every pixel writes its events from row base + workgroup offset +
//                prefix on.  With frame time stamps that is the final order and the events go straight to the caller's
//                arrays; with linear ones (k, (x, y, polarity)) pairs go to the workspace, k = t - T[0].
//   rocprim::radix_sort_pairs + k_ef_unpack   linear time stamps: the emitted order is (frame, polarity, y, x, j) and the
//                wanted one is a stable sort of it by t alone, over the key bits T[n-1] - T[0] needs; the sorted pairs are
//                unpacked into the caller's arrays.
//
// No float anywhere and no atomics: every offset is a sum of integers in a fixed order, so two runs give the same bits.
// Counts are 64-bit and the scans saturate, so no stream -- whatever the caller's reference plane holds -- can wrap a
// total: the emit pass writes only when the total it has formed itself equals the one the caller sized the outputs for.
#include <rocprim/device/device_radix_sort.hpp>

#include "nsof_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int EF_WG = 256;      // pixels per workgroup
constexpr int EF_BATCH = 4;     // frames whose loads are issued before the first of them is consumed
constexpr int EF_LUT_MAX = 1 << 30;

// What both passes read.
struct ef_args {
    const uint8_t* frames;
    ptrdiff_t rs, fs;         // row and frame stride, bytes
    int n, W, npx;            // frames, width, H * W
    const int32_t* lut;       // DEVICE [256]
    const int64_t* times;     // DEVICE [n]
    int c_on, c_off;          // the scalar thresholds (thr == nullptr)
    const int32_t* thr;       // DEVICE [H][W][2] (c_on, c_off) or nullptr
    const int32_t* ref_in;    // DEVICE [H][W] (ref_mode NSOF_EVENTS_REF_GIVEN)
    int ref_mode;
};

// A thread's pixel.  A thread past the last pixel walks pixel 0 (every load stays inside the frames and none is
// predicated) and counts nothing.
struct ef_px {
    bool in;
    const uint8_t* p;         // the pixel in frame 0
    int pix, x, y, c_on, c_off, r;
};

__device__ __forceinline__ ef_px ef_init(const ef_args& a, int (&sh_lut)[256])
{
    sh_lut[threadIdx.x] = a.lut[threadIdx.x];
    __syncthreads();
    ef_px q;
    const long long pix = (long long)blockIdx.x * EF_WG + threadIdx.x;
    q.in = pix < a.npx;
    q.pix = q.in ? (int)pix : 0;
    q.y = q.pix / a.W;
    q.x = q.pix - q.y * a.W;
    q.p = a.frames + (ptrdiff_t)q.y * a.rs + q.x;
    q.c_on = a.thr ? a.thr[2 * (size_t)q.pix] : a.c_on;
    q.c_off = a.thr ? a.thr[2 * (size_t)q.pix + 1] : a.c_off;
    q.r = a.ref_mode == NSOF_EVENTS_REF_GIVEN ? a.ref_in[q.pix] : a.ref_mode == NSOF_EVENTS_REF_FIRST ? sh_lut[*q.p] : 0;
    return q;
}

// The frames k0 .. k0 + EF_BATCH - 1 of the pixel (past the last frame: the last one again, unused).
__device__ __forceinline__ void ef_load(const ef_args& a, const ef_px& q, int k0, unsigned (&f)[EF_BATCH])
{
#pragma unroll
    for (int j = 0; j < EF_BATCH; j++) f[j] = q.p[(ptrdiff_t)min(k0 + j, a.n - 1) * a.fs];
}

// One step of r to the level b: the number of events (0 for a threshold < 1, which the entries refuse) and their
// polarity.  |b - r| < 2^32 for any int32 r, so the quotient and m * c fit 32 bits; r moves towards b and stays an int32.
__device__ __forceinline__ unsigned ef_step(int& r, int b, int c_on, int c_off, bool& on)
{
    const long long d = (long long)b - (long long)r;
    on = d > 0;
    const unsigned ad = (unsigned)(d < 0 ? -d : d);
    const int c = on ? c_on : c_off;
    const unsigned m = c >= 1 ? ad / (unsigned)c : 0u;
    const unsigned step = m * (unsigned)c;
    r = (int)(on ? (unsigned)r + step : (unsigned)r - step);
    return m;
}

// Inclusive prefix sum over the 64 lanes of a wave (every lane active) by DPP moves, without the LDS crossbar a shuffle
// goes through: within the rows of 16 lanes by shifts of 1, 2, 4 and 8, then lane 15 of rows 0 and 2 into rows 1 and 3,
// then lane 31 into rows 2 and 3.  A lane without a source adds 0.  Lane 63 holds the wave's sum.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned ef_dpp(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ unsigned ef_wave_scan(unsigned v)
{
    v += ef_dpp<0x111, 0xf>(v);   // row_shr:1
    v += ef_dpp<0x112, 0xf>(v);   // row_shr:2
    v += ef_dpp<0x114, 0xf>(v);   // row_shr:4
    v += ef_dpp<0x118, 0xf>(v);   // row_shr:8
    v += ef_dpp<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v += ef_dpp<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ unsigned ef_wave_last(unsigned v) { return (unsigned)__builtin_amdgcn_readlane((int)v, 63); }

__device__ __forceinline__ u64 sat_add(u64 a, u64 b)
{
    const u64 s = a + b;
    return s < a ? ~0ull : s;
}

__global__ __launch_bounds__(EF_WG) void k_ef_count(ef_args a, u64* __restrict__ table, u64* __restrict__ bad)
{
    __shared__ int sh_lut[256];
    __shared__ u64 sh[2][EF_BATCH][2][4];   // [set][frame of the batch][polarity][wave]; two sets used in turn: one barrier per batch
    ef_px q = ef_init(a, sh_lut);
    if (q.in && (q.c_on < 1 || q.c_off < 1)) *bad = 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n_wg = gridDim.x;
    int set = 0;
    for (int k0 = 0; k0 < a.n; k0 += EF_BATCH, set ^= 1) {
        unsigned f[EF_BATCH];
        ef_load(a, q, k0, f);
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            bool on = false;
            unsigned m = 0;
            if (k0 + j < a.n) m = ef_step(q.r, sh_lut[f[j]], q.c_on, q.c_off, on);
            if (!q.in) m = 0;
            u64 s_on, s_off;
            if (!__any(m >> 24)) {   // every lane below 2^24 (any frame of the linear table): the wave's sums fit 32 bits
                s_on = ef_wave_last(ef_wave_scan(on ? m : 0u));
                s_off = ef_wave_last(ef_wave_scan(on ? 0u : m));
            } else {
                s_on = on ? m : 0u;
                s_off = on ? 0u : m;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    s_on += __shfl_xor(s_on, o, 64);
                    s_off += __shfl_xor(s_off, o, 64);
                }
            }
            if (lane == 0) {
                sh[set][j][0][wave] = s_on;
                sh[set][j][1][wave] = s_off;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < 2 * EF_BATCH) {
            const int j = threadIdx.x >> 1, pol = threadIdx.x & 1;
            if (k0 + j < a.n)
                table[((size_t)(k0 + j) * 2 + pol) * n_wg + blockIdx.x] =
                    ((sh[set][j][pol][0] + sh[set][j][pol][1]) + sh[set][j][pol][2]) + sh[set][j][pol][3];
        }
    }
}

// Row blockIdx.x of data [rows][len]: exclusive prefix sums in place, the row's sum to tot[row].  Saturating.
__global__ __launch_bounds__(EF_WG) void k_ef_scan(u64* __restrict__ data, size_t len, u64* __restrict__ tot)
{
    __shared__ u64 sh[4];
    u64* row = data + (size_t)blockIdx.x * len;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (size_t base = 0; base < len; base += EF_WG) {
        const size_t i = base + threadIdx.x;
        u64 incl = i < len ? row[i] : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const u64 up = __shfl_up(incl, o, 64);
            if (lane >= o) incl = sat_add(incl, up);
        }
        u64 excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0;
        if (lane == 63) sh[wave] = incl;
        __syncthreads();
        u64 before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            if (w < wave) before = sat_add(before, sh[w]);
            all = sat_add(all, sh[w]);
        }
        if (i < len) row[i] = sat_add(carry, sat_add(before, excl));
        carry = sat_add(carry, all);
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// meta: [0 .. 2n) the bases of the (frame, polarity) rows, [2n] the total, [2n + 1] the bad-threshold flag.
__device__ __forceinline__ bool ef_guard(const u64* meta, int n, u64 expected) { return meta[2 * (size_t)n] == expected && meta[2 * (size_t)n + 1] == 0; }

template <int LINEAR>
__global__ __launch_bounds__(EF_WG) void k_ef_emit(ef_args a, const u64* __restrict__ table, const u64* __restrict__ meta,
                                                   u64 expected, int p_on, int p_off, int16_t* __restrict__ ox,
                                                   int16_t* __restrict__ oy, int8_t* __restrict__ op, int64_t* __restrict__ ot,
                                                   u64* __restrict__ keys, unsigned* __restrict__ vals,
                                                   int32_t* __restrict__ ref_out)
{
    if (!ef_guard(meta, a.n, expected)) return;   // the same for every thread of the grid: nothing is written
    __shared__ int sh_lut[256];
    __shared__ unsigned sh[2][EF_BATCH][2][4];
    ef_px q = ef_init(a, sh_lut);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n_wg = gridDim.x;
    const int64_t t_first = a.times[0];
    int prev_level = 0;   // L[k - 1]
    int set = 0;
    for (int k0 = 0; k0 < a.n; k0 += EF_BATCH, set ^= 1) {
        unsigned f[EF_BATCH];
        ef_load(a, q, k0, f);
        unsigned m[EF_BATCH], excl[EF_BATCH];
        int r0[EF_BATCH], lev[EF_BATCH];
        bool on[EF_BATCH];
        u64 base[EF_BATCH][2];   // where the workgroup's ON and OFF events of each frame start (the same in every lane)
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            const size_t row = (size_t)min(k0 + j, a.n - 1) * 2;
            base[j][0] = meta[row] + table[row * n_wg + blockIdx.x];
            base[j][1] = meta[row + 1] + table[(row + 1) * n_wg + blockIdx.x];
        }
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            lev[j] = sh_lut[f[j]];
            r0[j] = q.r;
            on[j] = false;
            m[j] = 0;
            if (k0 + j < a.n) m[j] = ef_step(q.r, lev[j], q.c_on, q.c_off, on[j]);
            if (!q.in) m[j] = 0;
            // the total is below 2^31 (the guard), so 32 bits hold every prefix
            const unsigned i_on = ef_wave_scan(on[j] ? m[j] : 0u), i_off = ef_wave_scan(on[j] ? 0u : m[j]);
            if (lane == 63) {
                sh[set][j][0][wave] = i_on;
                sh[set][j][1][wave] = i_off;
            }
            excl[j] = (on[j] ? i_on : i_off) - m[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            const int k = k0 + j;
            if (k >= a.n) break;
            const int a_level = prev_level;
            prev_level = lev[j];
            const int pol = on[j] ? 0 : 1;
            unsigned before = 0;
#pragma unroll
            for (int w = 0; w < 4; w++)
                if (w < wave) before += sh[set][j][pol][w];
            if (m[j] == 0) continue;
            size_t at = (size_t)(on[j] ? base[j][0] : base[j][1]) + before + excl[j];
            const int64_t t_k = a.times[k];
            const bool linear = LINEAR && k > 0;
            const int64_t t_prev = linear ? a.times[k - 1] : t_k;
            const u64 dt = (u64)(t_k - t_prev);
            const long long span = (long long)lev[j] - (long long)a_level;
            const u64 den = (u64)(span < 0 ? -span : span);
            const int c = on[j] ? q.c_on : q.c_off;
            const int8_t pv = (int8_t)(on[j] ? p_on : p_off);
            const unsigned packed = (unsigned)q.x | ((unsigned)q.y << 15) | (on[j] ? 1u << 30 : 0u);
            long long level = r0[j];
            for (unsigned i = 0; i < m[j]; i++, at++) {
                level += on[j] ? c : -c;
                int64_t t = t_k;
                if (linear && den) {
                    const long long off = level - (long long)a_level;
                    t = t_prev + (int64_t)(((u64)(off < 0 ? -off : off) * dt) / den);
                }
                if (LINEAR) {
                    keys[at] = (u64)(t - t_first);
                    vals[at] = packed;
                } else {
                    ox[at] = (int16_t)q.x;
                    oy[at] = (int16_t)q.y;
                    op[at] = pv;
                    ot[at] = t;
                }
            }
        }
    }
    if (q.in && ref_out) ref_out[q.pix] = q.r;
}

__global__ __launch_bounds__(EF_WG) void k_ef_unpack(size_t count, const u64* __restrict__ keys, const unsigned* __restrict__ vals,
                                                     const u64* __restrict__ meta, int n, u64 expected, int64_t t_first, int p_on,
                                                     int p_off, int16_t* __restrict__ ox, int16_t* __restrict__ oy,
                                                     int8_t* __restrict__ op, int64_t* __restrict__ ot)
{
    if (!ef_guard(meta, n, expected)) return;
    const size_t i = (size_t)blockIdx.x * EF_WG + threadIdx.x;
    if (i >= count) return;
    const unsigned v = vals[i];
    ox[i] = (int16_t)(v & 0x7fffu);
    oy[i] = (int16_t)((v >> 15) & 0x7fffu);
    op[i] = (int8_t)((v >> 30) ? p_on : p_off);
    ot[i] = (int64_t)keys[i] + t_first;
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct ef_call {
    const uint8_t* d_frames;
    ptrdiff_t row_stride, frame_stride;
    int n, H, W;
    const int64_t* times;
    const int32_t* lut;
    int c_on, c_off;
    const int32_t* d_thr;
    const int32_t* d_ref_in;
    int ref_mode;
};

// Every refusal of the arguments both entries share; nothing launched.
int ef_check(nsof_ctx* ctx, const char* who, const ef_call& c)
{
    if (c.n < 1 || c.H < 1 || c.W < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: %d frames of %dx%d", who, c.n, c.W, c.H);
    if (c.H > 32767 || c.W > 32767)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: %dx%d is beyond the int16 coordinates of an event (32767)", who, c.W, c.H);
    if (c.n > (1 << 24)) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%s: %d frames are beyond one launch (2^24)", who, c.n);
    if (!c.d_frames || !c.times || !c.lut)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (%s)", who, !c.d_frames ? "d_frames" : !c.times ? "times" : "lut");
    for (int k = 1; k < c.n; k++) {
        // the difference in unsigned arithmetic: times far apart must not overflow the check itself
        if (c.times[k] <= c.times[k - 1] || (unsigned long long)c.times[k] - (unsigned long long)c.times[k - 1] >= (1ull << 31))
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: times[%d] = %lld after times[%d] = %lld: the times must increase strictly, by "
                                  "less than 2^31", who, k, (long long)c.times[k], k - 1, (long long)c.times[k - 1]);
    }
    for (int i = 0; i < 256; i++)
        if (c.lut[i] < 0 || c.lut[i] > EF_LUT_MAX)
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: lut[%d] = %d is outside [0, 2^30]", who, i, c.lut[i]);
    if (!c.d_thr && (c.c_on < 1 || c.c_off < 1))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: thresholds c_on = %d, c_off = %d: both must be >= 1", who, c.c_on, c.c_off);
    if (c.ref_mode < NSOF_EVENTS_REF_ZERO || c.ref_mode > NSOF_EVENTS_REF_GIVEN || (c.ref_mode == NSOF_EVENTS_REF_GIVEN) != (c.d_ref_in != nullptr))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: ref_mode %d with d_ref_in %s", who, c.ref_mode, c.d_ref_in ? "given" : "NULL");
    return NSOF_OK;
}

// The workspace of a call, carved from ctx->tmp in one reservation.
struct ef_plan {
    ef_args args;
    size_t n_wg;
    u64 *table, *meta;        // [2n][n_wg]; [2n + 2]
    u64 *keys_in, *keys_out;  // linear time stamps: [count] each
    unsigned *vals_in, *vals_out;
    void* sort_tmp;
    size_t sort_bytes;
};

unsigned ef_key_bits(const ef_call& c)
{
    u64 span = (u64)c.times[c.n - 1] - (u64)c.times[0];
    unsigned bits = 1;
    while (bits < 64 && (span >> bits)) bits++;
    return bits;
}

// Uploads lut and times, reserves the workspace (sort_count > 0: with the buffers of the reorder) and queues the count pass
// and the two scans on ctx->stream.
int ef_count_pass(nsof_ctx* ctx, const ef_call& c, size_t sort_count, ef_plan* pl)
{
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t lut_bytes = 256 * sizeof(int32_t), tab_bytes = lut_bytes + (size_t)c.n * sizeof(int64_t);
    if (int rc = ctx->events.stage(ctx, tab_bytes, align_up(tab_bytes + tab_bytes / 2, 4096))) return rc;
    memcpy(ctx->events.h.p, c.lut, lut_bytes);
    memcpy((char*)ctx->events.h.p + lut_bytes, c.times, (size_t)c.n * sizeof(int64_t));
    const char* d_tab = (const char*)ctx->events.upload(ctx, tab_bytes);
    if (!d_tab) return NSOF_EDEVICE;

    const int npx = c.H * c.W;   // <= 32767^2 < 2^30
    pl->n_wg = (size_t)(npx + EF_WG - 1) / EF_WG;
    const size_t rows = 2 * (size_t)c.n;
    const size_t o_meta = align_up(rows * pl->n_wg * sizeof(u64), 256), o_keys = o_meta + align_up((rows + 2) * sizeof(u64), 256);
    size_t bytes = o_keys;
    pl->sort_bytes = 0;
    size_t o_keys_out = 0, o_vals = 0, o_vals_out = 0, o_sort = 0;
    if (sort_count) {
        NSOF_HIP(ctx, rocprim::radix_sort_pairs(nullptr, pl->sort_bytes, (const u64*)nullptr, (u64*)nullptr, (const unsigned*)nullptr,
                                                (unsigned*)nullptr, sort_count, 0u, ef_key_bits(c), ctx->stream));
        o_keys_out = o_keys + align_up(sort_count * sizeof(u64), 256);
        o_vals = o_keys_out + align_up(sort_count * sizeof(u64), 256);
        o_vals_out = o_vals + align_up(sort_count * sizeof(unsigned), 256);
        o_sort = o_vals_out + align_up(sort_count * sizeof(unsigned), 256);
        bytes = o_sort + pl->sort_bytes;
    }
    if (int rc = ctx->tmp.reserve(ctx, bytes)) return rc;
    char* ws = (char*)ctx->tmp.p;
    pl->table = (u64*)ws;
    pl->meta = (u64*)(ws + o_meta);
    pl->keys_in = (u64*)(ws + o_keys);
    pl->keys_out = (u64*)(ws + o_keys_out);
    pl->vals_in = (unsigned*)(ws + o_vals);
    pl->vals_out = (unsigned*)(ws + o_vals_out);
    pl->sort_tmp = ws + o_sort;

    ef_args& a = pl->args;
    a.frames = c.d_frames;
    a.rs = c.row_stride;
    a.fs = c.frame_stride;
    a.n = c.n;
    a.W = c.W;
    a.npx = npx;
    a.lut = (const int32_t*)d_tab;
    a.times = (const int64_t*)(d_tab + lut_bytes);
    a.c_on = c.c_on;
    a.c_off = c.c_off;
    a.thr = c.d_thr;
    a.ref_in = c.d_ref_in;
    a.ref_mode = c.ref_mode;

    NSOF_HIP(ctx, hipMemsetAsync(pl->meta + rows + 1, 0, sizeof(u64), ctx->stream));   // the bad-threshold flag
    hipLaunchKernelGGL(k_ef_count, dim3((unsigned)pl->n_wg), dim3(EF_WG), 0, ctx->stream, a, pl->table, pl->meta + rows + 1);
    NSOF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ef_scan, dim3((unsigned)rows), dim3(EF_WG), 0, ctx->stream, pl->table, pl->n_wg, pl->meta);
    NSOF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ef_scan, dim3(1), dim3(EF_WG), 0, ctx->stream, pl->meta, rows, pl->meta + rows);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

}  // namespace

extern "C" int nsof_events_from_frames_count_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                                 int n, int height, int width, const int64_t* times, const int32_t* lut, int c_on,
                                                 int c_off, const int32_t* d_thr_plane, const int32_t* d_ref_in, int ref_mode,
                                                 int64_t* frame_bounds_out)
{
    if (!ctx) return NSOF_EINVAL;
    const char* who = "events_from_frames_count";
    const ef_call c{d_frames, row_stride, frame_stride, n, height, width, times, lut, c_on, c_off, d_thr_plane, d_ref_in, ref_mode};
    if (int rc = ef_check(ctx, who, c)) return rc;
    if (!frame_bounds_out) return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (frame_bounds_out)", who);
    ef_plan pl;
    if (int rc = ef_count_pass(ctx, c, 0, &pl)) return rc;
    const size_t rows = 2 * (size_t)n;
    std::vector<u64> meta(rows + 2);
    NSOF_HIP(ctx, hipMemcpyAsync(meta.data(), pl.meta, meta.size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (meta[rows + 1])
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: the threshold plane holds a value < 1", who);
    if (meta[rows] >= (1ull << 31))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%s: %llu%s events, 2^31 or more", who, meta[rows], meta[rows] == ~0ull ? " or more" : "");
    for (int k = 0; k < n; k++) frame_bounds_out[k] = (int64_t)meta[2 * (size_t)k];
    frame_bounds_out[n] = (int64_t)meta[rows];
    return NSOF_OK;
}

extern "C" int nsof_events_from_frames_emit_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                                int n, int height, int width, const int64_t* times, const int32_t* lut, int c_on,
                                                int c_off, const int32_t* d_thr_plane, const int32_t* d_ref_in, int ref_mode,
                                                const int64_t* frame_bounds, int timestamps_mode, int p_on, int p_off,
                                                int64_t capacity, int16_t* d_x, int16_t* d_y, int8_t* d_p, int64_t* d_t,
                                                int32_t* d_ref_out)
{
    if (!ctx) return NSOF_EINVAL;
    const char* who = "events_from_frames_emit";
    const ef_call c{d_frames, row_stride, frame_stride, n, height, width, times, lut, c_on, c_off, d_thr_plane, d_ref_in, ref_mode};
    if (int rc = ef_check(ctx, who, c)) return rc;
    if (!frame_bounds) return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (frame_bounds)", who);
    if (timestamps_mode != NSOF_EVENTS_T_FRAME && timestamps_mode != NSOF_EVENTS_T_LINEAR)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: timestamps_mode %d", who, timestamps_mode);
    if (p_on < -128 || p_on > 127 || p_off < -128 || p_off > 127)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: p_on = %d, p_off = %d do not fit an int8", who, p_on, p_off);
    const int64_t total = frame_bounds[n];
    if (total < 0 || total >= (1ll << 31))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: frame_bounds[%d] = %lld is not a total the count entry gives", who, n, (long long)total);
    if (capacity < total)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: capacity %lld is below the %lld events of the stream", who, (long long)capacity,
                              (long long)total);
    if (total > 0 && (!d_x || !d_y || !d_p || !d_t))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (%s)", who, !d_x ? "d_x" : !d_y ? "d_y" : !d_p ? "d_p" : "d_t");
    const bool linear = timestamps_mode == NSOF_EVENTS_T_LINEAR && total > 0;
    ef_plan pl;
    if (int rc = ef_count_pass(ctx, c, linear ? (size_t)total : 0, &pl)) return rc;
    if (linear)
        hipLaunchKernelGGL(k_ef_emit<1>, dim3((unsigned)pl.n_wg), dim3(EF_WG), 0, ctx->stream, pl.args, pl.table, pl.meta, (u64)total, p_on,
                           p_off, d_x, d_y, d_p, d_t, pl.keys_in, pl.vals_in, d_ref_out);
    else
        hipLaunchKernelGGL(k_ef_emit<0>, dim3((unsigned)pl.n_wg), dim3(EF_WG), 0, ctx->stream, pl.args, pl.table, pl.meta, (u64)total, p_on,
                           p_off, d_x, d_y, d_p, d_t, pl.keys_in, pl.vals_in, d_ref_out);
    NSOF_HIP(ctx, hipGetLastError());
    if (linear) {
        NSOF_HIP(ctx, rocprim::radix_sort_pairs(pl.sort_tmp, pl.sort_bytes, (const u64*)pl.keys_in, pl.keys_out, (const unsigned*)pl.vals_in,
                                                pl.vals_out, (size_t)total, 0u, ef_key_bits(c), ctx->stream));
        hipLaunchKernelGGL(k_ef_unpack, dim3((unsigned)(((size_t)total + EF_WG - 1) / EF_WG)), dim3(EF_WG), 0, ctx->stream, (size_t)total,
                           pl.keys_out, pl.vals_out, pl.meta, n, (u64)total, times[0], p_on, p_off, d_x, d_y, d_p, d_t);
        NSOF_HIP(ctx, hipGetLastError());
    }
    return NSOF_OK;
}
