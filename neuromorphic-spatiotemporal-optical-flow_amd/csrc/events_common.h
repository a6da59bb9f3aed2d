// What the event generator (events_from_frames.hip) and the background-activity filter (events_denoise.hip) share: wave64,
// 256-thread workgroups, integers only, no atomics, a count / scan / guarded-scatter shape, and split entries that trust
// nothing they are handed.  The wave scan, the workgroup prefix, the table scan and the guard exist here once; so do the host
// checks of an event stream's arguments and the carving of ctx->tmp.
#pragma once

#include "nsof_internal.h"

namespace {

typedef unsigned long long u64;

constexpr int EV_WG = 256;   // threads of every workgroup: four waves
// A stream holds fewer than 2^31 events, which every entry checks: an event's index and every prefix of counts fit 32 bits.
constexpr long long EV_MAX_EVENTS = 1ll << 31;

// Inclusive prefix sum over the 64 lanes of a wave (every lane active) by DPP moves, without the LDS crossbar a shuffle
// goes through: within the rows of 16 lanes by shifts of 1, 2, 4 and 8, then lane 15 of rows 0 and 2 into rows 1 and 3,
// then lane 31 into rows 2 and 3.  A lane without a source adds 0.  Lane 63 holds the wave's sum.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned ev_dpp(unsigned v)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROW_MASK, 0xf, false);
}
__device__ __forceinline__ unsigned ev_wave_scan(unsigned v)
{
    v += ev_dpp<0x111, 0xf>(v);   // row_shr:1
    v += ev_dpp<0x112, 0xf>(v);   // row_shr:2
    v += ev_dpp<0x114, 0xf>(v);   // row_shr:4
    v += ev_dpp<0x118, 0xf>(v);   // row_shr:8
    v += ev_dpp<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v += ev_dpp<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return v;
}
__device__ __forceinline__ unsigned ev_wave_last(unsigned v) { return (unsigned)__builtin_amdgcn_readlane((int)v, 63); }

__device__ __forceinline__ u64 sat_add(u64 a, u64 b)
{
    const u64 s = a + b;
    return s < a ? ~0ull : s;
}
// The add of a scan: saturating (any u64) or plain (sums known to fit).
template <bool SAT, class T>
__device__ __forceinline__ T ev_add(T a, T b)
{
    if constexpr (SAT) return sat_add(a, b);
    else return a + b;
}

// The workgroup prefix from the waves' inclusive scans, in two pieces around a barrier that stays with the caller (who may
// put several sets before one barrier): lane 63 puts its wave's sum into sh[wave]; after the barrier every thread collects
// the sums of the earlier waves (before) and of all four (all).
template <class T>
__device__ __forceinline__ void ev_wg_put(T (&sh)[4], T incl) { if ((threadIdx.x & 63) == 63) sh[threadIdx.x >> 6] = incl; }
template <class T>
struct ev_wg_sums { T before, all; };
template <bool SAT = false, class T>
__device__ __forceinline__ ev_wg_sums<T> ev_wg_collect(const T (&sh)[4])
{
    const int wave = threadIdx.x >> 6;
    ev_wg_sums<T> s{0, 0};
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < wave) s.before = ev_add<SAT>(s.before, sh[w]);
        s.all = ev_add<SAT>(s.all, sh[w]);
    }
    return s;
}

// Row blockIdx.x of data [rows][len]: exclusive prefix sums in place, in index order, the row's sum to tot[row].  One
// workgroup per row, EV_WG entries at a time with a 64-bit carry.  SAT: the entries are any u64; the waves scan 64-bit
// values through shuffles and every add saturates.  Else a chunk's EV_WG entries must add up to less than 2^32: they are
// scanned in 32 bits by DPP moves with plain adds, and only the carry is 64-bit.
template <bool SAT>
__global__ __launch_bounds__(EV_WG) void k_ev_scan(u64* __restrict__ data, size_t len, u64* __restrict__ tot)
{
    typedef std::conditional_t<SAT, u64, unsigned> T;
    __shared__ T sh[4];
    u64* row = data + (size_t)blockIdx.x * len;
    const int lane = threadIdx.x & 63;
    u64 carry = 0;
    for (size_t base = 0; base < len; base += EV_WG) {
        const size_t i = base + threadIdx.x;
        const T v = i < len ? (T)row[i] : 0;
        T incl = v, excl;
        if constexpr (SAT) {
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 up = __shfl_up(incl, o, 64);
                if (lane >= o) incl = sat_add(incl, up);
            }
            excl = __shfl_up(incl, 1, 64);
            if (lane == 0) excl = 0;
        } else {
            incl = ev_wave_scan(v);
            excl = incl - v;
        }
        ev_wg_put(sh, incl);
        __syncthreads();
        const ev_wg_sums<T> s = ev_wg_collect<SAT>(sh);
        if (i < len) row[i] = ev_add<SAT>(carry, (u64)ev_add<SAT>(s.before, excl));
        carry = ev_add<SAT>(carry, (u64)s.all);
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = carry;
}

// The one test under which a second entry's kernels write: m[0], the total the call has formed itself, is the one the caller
// sized the outputs for, and neither of the two validation flags m[1], m[2] is up.  Sizes or a mask from another call cannot
// send a store past the outputs.  The same for every thread of the grid.
__device__ __forceinline__ bool ev_guard(const u64* m, u64 expected) { return m[0] == expected && m[1] == 0 && m[2] == 0; }

// ---- host ---------------------------------------------------------------------------------------------------------
// x and y are int16: a sensor's height and width lie in [1, 32767].  (The two files word the refusal differently.)
inline bool ev_sensor_ok(int H, int W) { return H >= 1 && W >= 1 && H <= 32767 && W <= 32767; }

// The refusal of a null pointer among the four arrays of a stream.
inline int ev_check_stream(nsof_ctx* ctx, const char* who, const void* d_x, const void* d_y, const void* d_p, const void* d_t)
{
    if (d_x && d_y && d_p && d_t) return NSOF_OK;
    return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (%s)", who, !d_x ? "d_x" : !d_y ? "d_y" : !d_p ? "d_p" : "d_t");
}

// The running carve of ctx->tmp: take(bytes) is the offset of the next array, 256-byte aligned; `at` what to reserve.
struct ev_carve {
    size_t at = 0;
    size_t take(size_t bytes) { return std::exchange(at, at + align_up(bytes, 256)); }
};

}  // namespace
