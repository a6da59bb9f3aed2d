// Background-activity filter for event streams (nsof_events_denoise_mark_dev / _compact_dev): the
// spatiotemporal correlation filter of the event-camera tool chains, all in integers.  `last` holds, per (channel, pixel),
// the time of the latest event seen there (INT64_MIN: never).  Event i at pixel q is kept iff at least min_support pixels n
// of the square of `radius` around q (clipped to the sensor; q itself only with include_self) have
// last[n] >= max(t_i - dt_us, INT64_MIN + 1); then last[q] = t_i, kept or not.  t never decreases over the stream, so
// last[n] at event i is the time of the latest event j < i at n, or the incoming plane's value: a decision depends on the
// input stream alone, and the sequential rule has an exact parallel form.
//
//   k_ed_keys    per event the 64-bit word (c * H * W + y * W + x) << 32 | i, c the channel; a coordinate outside the
//                sensor or t[i] < t[i-1] raises a flag and takes the key C * H * W, which no search looks for.
//   rocprim::radix_sort_keys over the key bits alone: the words enter in ascending i and the sort is stable, so they
//                leave in ascending (key, i) order -- each (channel, pixel) owns a segment of ascending stream indices.
//   k_ed_mark    a thread owns an event (thread j the j-th sorted word: neighbouring lanes search for neighbouring words) and,
//                per neighbour n, finds the last word below (key(n), i) by a binary search over
//                the whole sorted array (no table of segment offsets: the memory is in N, whatever the sensor's size; a
//                hot pixel's long segment costs log2 N steps like any other).  That word is the latest earlier event at
//                n, if its key is n's; else the incoming plane decides.  The searches of one row of the window run side by
//                side (2 * radius + 1 independent gathers per step).  Writes keep[i].
//   k_ed_count + k_ev_scan   the kept events of every 256 consecutive ones, then the exclusive prefix of those counts in
//                index order by one workgroup: the total.  k_ed_bounds: the kept count before each of the caller's bounds.
//   k_ed_compact every workgroup re-forms the prefix inside its 256 events and scatters the kept x, y, p, t: the input
//                order with the gaps closed.
//   k_ed_last_init + k_ed_last_set   last_out = last_in (or never), then the t of every segment's last word.
//
// The wave scan, the workgroup prefix, the table scan (k_ev_scan) and the guard are the event kernels' shared ones
// (events_common.h).  No float and no atomics: every offset is a sum of integers in a fixed order, so two runs give the same
// bits.  The compact entry trusts nothing it is handed: it validates the stream again, sorts again (for the segments' ends),
// counts the keep bytes itself, and all its kernels leave unless that total equals the capacity the outputs were sized for and
// no validation flag is up (ev_guard on meta).
#include <rocprim/device/device_radix_sort.hpp>

#include "events_common.h"

namespace {

constexpr int ED_WG = EV_WG;   // threads of every workgroup; the count and compact kernels own ED_WG consecutive events (a chunk)
// meta: [0] the kept total, [1] a coordinate outside the sensor, [2] a decreasing t
constexpr int ED_META = 4;

struct ed_stream {
    const int16_t *x, *y;
    const int8_t* p;
    const int64_t* t;
    unsigned n;               // events, < 2^31
    int H, W;
    unsigned plane;           // H * W
    int channels;             // 2 with same_polarity
};

__global__ __launch_bounds__(ED_WG) void k_ed_keys(ed_stream s, u64* __restrict__ words, u64* __restrict__ meta)
{
    const unsigned i = blockIdx.x * ED_WG + threadIdx.x;
    if (i >= s.n) return;
    const int x = s.x[i], y = s.y[i];
    const bool bad_xy = (unsigned)x >= (unsigned)s.W || (unsigned)y >= (unsigned)s.H;
    const bool bad_t = i > 0 && s.t[i] < s.t[i - 1];
    if (bad_xy) meta[1] = 1;
    if (bad_t) meta[2] = 1;
    const unsigned c = s.channels == 2 && s.p[i] <= 0 ? 1u : 0u;
    const unsigned key = bad_xy || bad_t ? (unsigned)s.channels * s.plane : c * s.plane + (unsigned)y * (unsigned)s.W + (unsigned)x;
    words[i] = (u64)key << 32 | i;
}

struct ed_rule {
    long long dt;             // [0, 2^31)
    int min_support, include_self;
    const int64_t* last_in;   // DEVICE [C][H][W] or nullptr: never
};

// The number of sorted words below `target`, for R2 = 2 * R + 1 targets at once: `top` is the largest power of two <= n.
template <int R2>
__device__ __forceinline__ void ed_search(const u64* __restrict__ sorted, unsigned n, unsigned top, const u64 (&target)[R2], unsigned (&pos)[R2])
{
#pragma unroll
    for (int d = 0; d < R2; d++) pos[d] = 0;
    for (unsigned step = top; step; step >>= 1) {
#pragma unroll
        for (int d = 0; d < R2; d++) {
            const unsigned to = pos[d] + step;   // < 2^32: pos < n < 2^31, step <= 2^30
            if (to <= n && sorted[to - 1] < target[d]) pos[d] = to;
        }
    }
}

template <int R>
__global__ __launch_bounds__(ED_WG) void k_ed_mark(ed_stream s, ed_rule r, const u64* __restrict__ sorted, unsigned top,
                                                   const u64* __restrict__ meta, uint8_t* __restrict__ keep)
{
    if (meta[1] | meta[2]) return;   // a refused stream: nothing is addressed and nothing written
    const unsigned j = blockIdx.x * ED_WG + threadIdx.x;
    if (j >= s.n) return;
    constexpr int R2 = 2 * R + 1;
    // the events in sorted order: the lanes of a wave sit at one pixel or at neighbours, so their searches walk the same lines
    const u64 own = sorted[j];
    const unsigned i = (unsigned)own, k = (unsigned)(own >> 32);
    const unsigned base = k >= s.plane ? s.plane : 0u;   // the channel's plane (no flag is up: k < C * H * W)
    const int y = (int)((k - base) / (unsigned)s.W), x = (int)((k - base) - (unsigned)y * (unsigned)s.W);
    const int64_t t = s.t[i];
    const int64_t lo = t < INT64_MIN + 1 + r.dt ? INT64_MIN + 1 : t - r.dt;   // max(t - dt, INT64_MIN + 1) without a wrap
    int support = 0;
    for (int dy = -R; dy <= R && support < r.min_support; dy++) {
        const int ny = y + dy;
        if (ny < 0 || ny >= s.H) continue;
        bool in[R2];
        unsigned key[R2];
        u64 target[R2];
        unsigned pos[R2];
#pragma unroll
        for (int d = 0; d < R2; d++) {
            const int nx = x + d - R;
            in[d] = nx >= 0 && nx < s.W && (r.include_self || dy != 0 || d != R);
            key[d] = in[d] ? base + (unsigned)ny * (unsigned)s.W + (unsigned)nx : 0u;
            target[d] = in[d] ? (u64)key[d] << 32 | i : 0ull;   // nothing is below 0: a search that gathers from one line
        }
        ed_search<R2>(sorted, s.n, top, target, pos);
#pragma unroll
        for (int d = 0; d < R2; d++) {
            if (!in[d]) continue;
            const u64 w = pos[d] ? sorted[pos[d] - 1] : ~0ull;   // (no key is 2^32 - 1)
            int64_t tl = INT64_MIN;
            if ((unsigned)(w >> 32) == key[d]) tl = s.t[(unsigned)w];   // the latest earlier event of the call at n
            else if (r.last_in) tl = r.last_in[key[d]];
            support += tl >= lo;
        }
    }
    keep[i] = support >= r.min_support;
}

// Whether the thread's event of the chunk is kept (one below `limit` only), the kept events of the workgroup's earlier
// threads (excl) and of the whole workgroup (all).  Every thread of the workgroup calls it.
__device__ __forceinline__ bool ed_chunk_prefix(const uint8_t* __restrict__ keep, size_t chunk, size_t limit, unsigned (&sh)[4],
                                                unsigned& excl, unsigned& all)
{
    const size_t i = chunk * ED_WG + threadIdx.x;
    const bool kept = i < limit && keep[i] != 0;
    const unsigned incl = ev_wave_scan(kept);
    ev_wg_put(sh, incl);
    __syncthreads();
    const ev_wg_sums<unsigned> s = ev_wg_collect(sh);
    all = s.all;
    excl = s.before + incl - kept;
    return kept;
}

__global__ __launch_bounds__(ED_WG) void k_ed_count(const uint8_t* __restrict__ keep, size_t n, u64* __restrict__ table)
{
    __shared__ unsigned sh[4];
    unsigned excl, all;
    ed_chunk_prefix(keep, blockIdx.x, n, sh, excl, all);
    if (threadIdx.x == 0) table[blockIdx.x] = all;
}

// out[k]: the kept events before bounds[k] (in [0, n], checked by the entry).  One workgroup per bound.
__global__ __launch_bounds__(ED_WG) void k_ed_bounds(const uint8_t* __restrict__ keep, size_t n, const u64* __restrict__ table,
                                                     const u64* __restrict__ meta, const int64_t* __restrict__ bounds,
                                                     int64_t* __restrict__ out)
{
    __shared__ unsigned sh[4];
    const size_t b = (size_t)bounds[blockIdx.x];
    if (b >= n) {   // (the same in every thread)
        if (threadIdx.x == 0) out[blockIdx.x] = (int64_t)meta[0];
        return;
    }
    unsigned excl, all;
    ed_chunk_prefix(keep, b / ED_WG, b, sh, excl, all);
    if (threadIdx.x == 0) out[blockIdx.x] = (int64_t)(table[b / ED_WG] + all);
}

struct ed_out {
    int16_t *x, *y;
    int8_t* p;
    int64_t* t;
};

__global__ __launch_bounds__(ED_WG) void k_ed_compact(ed_stream s, const uint8_t* __restrict__ keep, const u64* __restrict__ table,
                                                      const u64* __restrict__ meta, u64 expected, ed_out o)
{
    if (!ev_guard(meta, expected)) return;
    __shared__ unsigned sh[4];
    unsigned excl, all;
    if (!ed_chunk_prefix(keep, blockIdx.x, s.n, sh, excl, all)) return;
    const size_t i = (size_t)blockIdx.x * ED_WG + threadIdx.x;
    const size_t at = (size_t)table[blockIdx.x] + excl;   // below the total, which is the outputs' size
    o.x[at] = s.x[i];
    o.y[at] = s.y[i];
    o.p[at] = s.p[i];
    o.t[at] = s.t[i];
}

__global__ __launch_bounds__(ED_WG) void k_ed_last_init(size_t count, const int64_t* __restrict__ last_in, const u64* __restrict__ meta,
                                                        u64 expected, int64_t* __restrict__ last_out)
{
    if (!ev_guard(meta, expected)) return;
    const size_t i = (size_t)blockIdx.x * ED_WG + threadIdx.x;
    if (i < count) last_out[i] = last_in ? last_in[i] : INT64_MIN;
}

// The last word of every segment: the latest event of its (channel, pixel).
__global__ __launch_bounds__(ED_WG) void k_ed_last_set(ed_stream s, const u64* __restrict__ sorted, const u64* __restrict__ meta,
                                                       u64 expected, int64_t* __restrict__ last_out)
{
    if (!ev_guard(meta, expected)) return;   // (no flag is up: every key is below C * H * W)
    const unsigned j = blockIdx.x * ED_WG + threadIdx.x;
    if (j >= s.n) return;
    const u64 w = sorted[j];
    const unsigned key = (unsigned)(w >> 32);
    if (j + 1 < s.n && (unsigned)(sorted[j + 1] >> 32) == key) return;
    last_out[key] = s.t[(unsigned)w];
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct ed_call {
    const int16_t *d_x, *d_y;
    const int8_t* d_p;
    const int64_t* d_t;
    int64_t n;
    int H, W, same_polarity;
    const int64_t* d_last_in;
};

// Every refusal of the arguments both entries share; nothing launched.
int ed_check(nsof_ctx* ctx, const char* who, const ed_call& c)
{
    if (c.n < 0 || c.n >= EV_MAX_EVENTS) return nsof_set_error(ctx, NSOF_EINVAL, "%s: n = %lld is outside [0, 2^31)", who, (long long)c.n);
    if (!ev_sensor_ok(c.H, c.W))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: a %dx%d sensor; height and width lie in [1, 32767], the int16 coordinates of an event",
                              who, c.W, c.H);
    if (c.same_polarity != 0 && c.same_polarity != 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: same_polarity = %d is neither 0 nor 1", who, c.same_polarity);
    return c.n > 0 ? ev_check_stream(ctx, who, c.d_x, c.d_y, c.d_p, c.d_t) : NSOF_OK;
}

// The workspace of a call, carved from ctx->tmp in one reservation.
struct ed_plan {
    ed_stream s;
    unsigned key_bits, n_wg, top;   // n_wg: the chunks, and the workgroups of the per-event kernels
    u64 *words, *sorted, *table, *meta;
    int64_t* bounds_out;
    void* sort_tmp;
    size_t sort_bytes;
};

// (the entry has made ctx->device current)
int ed_reserve(nsof_ctx* ctx, const ed_call& c, size_t n_bounds, ed_plan* pl)
{
    ed_stream& s = pl->s;
    s = ed_stream{c.d_x, c.d_y, c.d_p, c.d_t, (unsigned)c.n, c.H, c.W, (unsigned)c.H * (unsigned)c.W, c.same_polarity ? 2 : 1};
    const unsigned sentinel = (unsigned)s.channels * s.plane;   // <= 2 * 32767^2 < 2^31
    pl->key_bits = 1;
    while (sentinel >> pl->key_bits) pl->key_bits++;
    pl->n_wg = (unsigned)(((size_t)c.n + ED_WG - 1) / ED_WG);
    pl->top = 1;
    while ((u64)pl->top * 2 <= s.n) pl->top *= 2;
    pl->sort_bytes = 0;
    if (c.n)
        NSOF_HIP(ctx, rocprim::radix_sort_keys(nullptr, pl->sort_bytes, (const u64*)nullptr, (u64*)nullptr, (size_t)c.n, 32u,
                                               32u + pl->key_bits, ctx->stream));
    ev_carve w;
    const size_t o_words = w.take((size_t)c.n * sizeof(u64)), o_sorted = w.take((size_t)c.n * sizeof(u64));
    const size_t o_table = w.take((size_t)pl->n_wg * sizeof(u64)), o_meta = w.take(ED_META * sizeof(u64));
    const size_t o_bounds = w.take(n_bounds * sizeof(int64_t)), o_sort = w.at;
    if (int rc = ctx->tmp.reserve(ctx, o_sort + pl->sort_bytes)) return rc;
    char* ws = (char*)ctx->tmp.p;
    pl->words = (u64*)(ws + o_words);
    pl->sorted = (u64*)(ws + o_sorted);
    pl->table = (u64*)(ws + o_table);
    pl->meta = (u64*)(ws + o_meta);
    pl->bounds_out = (int64_t*)(ws + o_bounds);
    pl->sort_tmp = ws + o_sort;
    return NSOF_OK;
}

// Validation and the sorted words, queued on ctx->stream.  n > 0.
int ed_sort_pass(nsof_ctx* ctx, const ed_plan& pl)
{
    NSOF_HIP(ctx, hipMemsetAsync(pl.meta, 0, ED_META * sizeof(u64), ctx->stream));
    hipLaunchKernelGGL(k_ed_keys, dim3(pl.n_wg), dim3(ED_WG), 0, ctx->stream, pl.s, pl.words, pl.meta);
    NSOF_HIP(ctx, hipGetLastError());
    size_t bytes = pl.sort_bytes;
    NSOF_HIP(ctx, rocprim::radix_sort_keys(pl.sort_tmp, bytes, (const u64*)pl.words, pl.sorted, (size_t)pl.s.n, 32u, 32u + pl.key_bits,
                                           ctx->stream));
    return NSOF_OK;
}

// The chunk counts of `keep`, their exclusive prefix and the total (meta[0]).  n > 0.
int ed_count_pass(nsof_ctx* ctx, const ed_plan& pl, const uint8_t* d_keep)
{
    hipLaunchKernelGGL(k_ed_count, dim3(pl.n_wg), dim3(ED_WG), 0, ctx->stream, d_keep, (size_t)pl.s.n, pl.table);
    NSOF_HIP(ctx, hipGetLastError());
    // one row; an entry is a chunk's count, at most ED_WG, so the ED_WG entries of a scan step add up to at most 2^16
    hipLaunchKernelGGL(k_ev_scan<false>, dim3(1), dim3(ED_WG), 0, ctx->stream, pl.table, (size_t)pl.n_wg, pl.meta);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

}  // namespace

extern "C" int nsof_events_denoise_mark_dev(nsof_ctx* ctx, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                                            int64_t n, int height, int width, int64_t dt_us, int radius, int min_support,
                                            int same_polarity, int include_self, const int64_t* d_last_in, const int64_t* bounds,
                                            int64_t n_bounds, uint8_t* d_keep, int64_t* n_kept_out, int64_t* bounds_out)
{
    if (!ctx) return NSOF_EINVAL;
    const char* who = "events_denoise_mark";
    const ed_call c{d_x, d_y, d_p, d_t, n, height, width, same_polarity, d_last_in};
    if (int rc = ed_check(ctx, who, c)) return rc;
    if (dt_us < 0 || dt_us >= (1ll << 31)) return nsof_set_error(ctx, NSOF_EINVAL, "%s: dt_us = %lld is outside [0, 2^31)", who, (long long)dt_us);
    if (radius != 1 && radius != 2) return nsof_set_error(ctx, NSOF_EINVAL, "%s: radius = %d; 1 or 2 expected", who, radius);
    if (min_support < 1 || min_support > (2 * radius + 1) * (2 * radius + 1))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: min_support = %d is outside [1, %d], the pixels of the window", who, min_support,
                              (2 * radius + 1) * (2 * radius + 1));
    if (include_self != 0 && include_self != 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: include_self = %d is neither 0 nor 1", who, include_self);
    if (!n_kept_out || (n > 0 && !d_keep)) return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (%s)", who, !n_kept_out ? "n_kept_out" : "d_keep");
    if (n_bounds < 0 || n_bounds > (1ll << 24) || (n_bounds > 0 && (!bounds || !bounds_out)))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: %lld bounds with bounds %s and bounds_out %s; at most 2^24, both arrays given", who,
                              (long long)n_bounds, bounds ? "given" : "NULL", bounds_out ? "given" : "NULL");
    for (int64_t k = 0; k < n_bounds; k++)
        if (bounds[k] < (k ? bounds[k - 1] : 0) || bounds[k] > n)
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: bounds[%lld] = %lld: the bounds must not decrease and lie in [0, %lld]", who,
                                  (long long)k, (long long)bounds[k], (long long)n);
    if (n == 0) {   // nothing to launch: no kernel indexes an empty array
        *n_kept_out = 0;
        for (int64_t k = 0; k < n_bounds; k++) bounds_out[k] = 0;
        return NSOF_OK;
    }
    NSOF_HIP(ctx, hipSetDevice(ctx->device));   // before the staging below creates its event and its two copies
    const int64_t* d_bounds = nullptr;
    if (n_bounds) {
        const size_t bytes = (size_t)n_bounds * sizeof(int64_t);
        if (int rc = ctx->events.stage(ctx, bytes, align_up(bytes + bytes / 2, 4096))) return rc;
        memcpy(ctx->events.h.p, bounds, bytes);
        if (!(d_bounds = (const int64_t*)ctx->events.upload(ctx, bytes))) return NSOF_EDEVICE;
    }
    ed_plan pl;
    if (int rc = ed_reserve(ctx, c, (size_t)n_bounds, &pl)) return rc;
    if (int rc = ed_sort_pass(ctx, pl)) return rc;
    const ed_rule r{dt_us, min_support, include_self, d_last_in};
    nsof_with_int<1, 2>(radius, [&](auto tag) {
        hipLaunchKernelGGL(k_ed_mark<decltype(tag)::value>, dim3(pl.n_wg), dim3(ED_WG), 0, ctx->stream, pl.s, r, (const u64*)pl.sorted,
                           pl.top, (const u64*)pl.meta, d_keep);
    });
    NSOF_HIP(ctx, hipGetLastError());
    if (int rc = ed_count_pass(ctx, pl, d_keep)) return rc;
    if (n_bounds) {
        hipLaunchKernelGGL(k_ed_bounds, dim3((unsigned)n_bounds), dim3(ED_WG), 0, ctx->stream, (const uint8_t*)d_keep, (size_t)n,
                           (const u64*)pl.table, (const u64*)pl.meta, d_bounds, pl.bounds_out);
        NSOF_HIP(ctx, hipGetLastError());
    }
    u64 meta[ED_META];
    std::vector<int64_t> kept_before((size_t)n_bounds);
    NSOF_HIP(ctx, hipMemcpyAsync(meta, pl.meta, sizeof(meta), hipMemcpyDeviceToHost, ctx->stream));
    if (n_bounds)
        NSOF_HIP(ctx, hipMemcpyAsync(kept_before.data(), pl.bounds_out, (size_t)n_bounds * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (meta[1]) return nsof_set_error(ctx, NSOF_EINVAL, "%s: an event lies outside the %dx%d sensor", who, width, height);
    if (meta[2]) return nsof_set_error(ctx, NSOF_EINVAL, "%s: t decreases somewhere in the stream", who);
    *n_kept_out = (int64_t)meta[0];
    for (int64_t k = 0; k < n_bounds; k++) bounds_out[k] = kept_before[(size_t)k];
    return NSOF_OK;
}

extern "C" int nsof_events_denoise_compact_dev(nsof_ctx* ctx, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p,
                                               const int64_t* d_t, int64_t n, int height, int width, int same_polarity,
                                               const int64_t* d_last_in, const uint8_t* d_keep, int64_t capacity, int16_t* d_x_out,
                                               int16_t* d_y_out, int8_t* d_p_out, int64_t* d_t_out, int64_t* d_last_out)
{
    if (!ctx) return NSOF_EINVAL;
    const char* who = "events_denoise_compact";
    const ed_call c{d_x, d_y, d_p, d_t, n, height, width, same_polarity, d_last_in};
    if (int rc = ed_check(ctx, who, c)) return rc;
    if (capacity < 0 || capacity > n)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: capacity %lld is not a kept count of %lld events", who, (long long)capacity, (long long)n);
    if (n > 0 && !d_keep) return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (d_keep)", who);
    if (capacity > 0 && (!d_x_out || !d_y_out || !d_p_out || !d_t_out))
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (%s)", who, !d_x_out ? "d_x_out" : !d_y_out ? "d_y_out" : !d_p_out ? "d_p_out" : "d_t_out");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    ed_plan pl;
    if (int rc = ed_reserve(ctx, c, 0, &pl)) return rc;
    if (n == 0) {
        NSOF_HIP(ctx, hipMemsetAsync(pl.meta, 0, ED_META * sizeof(u64), ctx->stream));   // a total of 0 and no flag
    } else {
        if (int rc = ed_sort_pass(ctx, pl)) return rc;
        if (int rc = ed_count_pass(ctx, pl, d_keep)) return rc;
        hipLaunchKernelGGL(k_ed_compact, dim3(pl.n_wg), dim3(ED_WG), 0, ctx->stream, pl.s, d_keep, (const u64*)pl.table,
                           (const u64*)pl.meta, (u64)capacity, ed_out{d_x_out, d_y_out, d_p_out, d_t_out});
        NSOF_HIP(ctx, hipGetLastError());
    }
    if (d_last_out) {
        const size_t count = (size_t)pl.s.channels * pl.s.plane;
        if (d_last_out != d_last_in) {
            hipLaunchKernelGGL(k_ed_last_init, dim3((unsigned)((count + ED_WG - 1) / ED_WG)), dim3(ED_WG), 0, ctx->stream, count, d_last_in,
                               (const u64*)pl.meta, (u64)capacity, d_last_out);
            NSOF_HIP(ctx, hipGetLastError());
        }
        if (n > 0) {
            hipLaunchKernelGGL(k_ed_last_set, dim3(pl.n_wg), dim3(ED_WG), 0, ctx->stream, pl.s, (const u64*)pl.sorted, (const u64*)pl.meta,
                               (u64)capacity, d_last_out);
            NSOF_HIP(ctx, hipGetLastError());
        }
    }
    return NSOF_OK;
}
