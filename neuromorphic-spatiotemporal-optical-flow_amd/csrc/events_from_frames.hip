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
//   k_ev_scan    an exclusive scan of every row of that table in place (one workgroup per row, 256 entries at a time)
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
//
// The sensor entries (nsof_events_from_frames_sensor_*_dev) run the SENSOR instantiations of the
// count and emit kernels: per pixel and frame one Philox block gives up to two noise candidates, and -- with a refractory
// time or a given t_ok plane -- the pixel's candidates are walked in time order against t_ok, which lives in a register
// like r.  The count pass runs the same walk as the emit pass, so its counts depend on the stamp mode.  The plain
// instantiations hold none of this.
//
// What the two passes must agree on exists once: ef_frame builds a frame's candidates (the level step, and with SENSOR the
// times and the noise draw) for k_ef_count and for the sensor emit body, ef_survivors counts them (without SENSOR: the
// candidates themselves), ef_stamp is the linear stamp of a crossing, ef_store writes an event, ef_bases forms a batch's row
// bases and ev_guard is the one test under which the emit and unpack kernels write.  The wave scan, the workgroup prefix, the
// table scan and the guard are the event kernels' shared ones (events_common.h).  The emit pass keeps two bodies,
// ef_emit_plain and ef_emit_sensor: folded into one, the plain linear kernel went from 64 to 90 VGPRs.
#include <rocprim/device/device_radix_sort.hpp>

#include "accum_c2c.h"
#include "events_common.h"

namespace {

constexpr int EF_WG = EV_WG;    // pixels per workgroup
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

// What the SENSOR instantiations read besides (the plain ones take it and leave it alone).
constexpr unsigned EF_NOISE_WORD = 0x4E534546u;   // the fourth counter word: apart from the c2c draws of the same seed
constexpr unsigned EF_NONE = 0xffffffffu;         // no noise candidate (an offset into the interval is below 2^31)
constexpr unsigned EF_WALK_MAX = 1u << 20;        // crossings of one step a thread walks one by one
struct ef_sensor {
    long long refractory;     // microseconds, [0, 2^31)
    long long first_frame;    // the absolute index of frame 0
    unsigned k0, k1;          // the Philox key: the seed's two words
    unsigned rate_on, rate_off;   // 2^-32 per microsecond (rate_plane == nullptr)
    const unsigned* rate_plane;   // DEVICE [H][W][2] or nullptr
    const int64_t* t_ok_in;   // DEVICE [H][W] or nullptr: every pixel starts at INT64_MIN
    int noise;                // some rate may be non-zero
    int walk;                 // a candidate may be dropped: refractory > 0 or t_ok_in given
    int linear;               // the stamp mode (the count pass; the emit pass has it as a template argument)
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

// ---- the sensor model (SENSOR instantiations only) ------------------------------------------------------------------
// A pixel's sensor state: its noise rates and t_ok, the earliest time at which it may fire again.
struct ef_spx {
    unsigned rate_on, rate_off;
    int64_t t_ok;
};

__device__ __forceinline__ ef_spx ef_sensor_init(const ef_sensor& s, const ef_px& q)
{
    ef_spx p;
    p.rate_on = s.rate_plane ? s.rate_plane[2 * (size_t)q.pix] : s.rate_on;
    p.rate_off = s.rate_plane ? s.rate_plane[2 * (size_t)q.pix + 1] : s.rate_off;
    p.t_ok = s.t_ok_in ? s.t_ok_in[q.pix] : INT64_MIN;
    return p;
}

// The noise candidates of a pixel in the interval before frame k >= 1 of the call, dt = T[k] - T[k-1] < 2^31: their
// offsets from T[k-1], EF_NONE for none.  One Philox block; a silent pixel draws nothing.
__device__ __forceinline__ void ef_noise(const ef_sensor& s, const ef_px& q, const ef_spx& p, int k, u64 dt, unsigned& off_on,
                                         unsigned& off_off)
{
    off_on = off_off = EF_NONE;
    if (!(p.rate_on | p.rate_off)) return;
    const u64 f = (u64)(s.first_frame + k);
    unsigned c[4] = {(unsigned)q.pix, (unsigned)f, (unsigned)(f >> 32), EF_NOISE_WORD};
    philox4x32_10(c, s.k0, s.k1);
    const u64 p_on = min((u64)p.rate_on * dt, 0xffffffffull), p_off = min((u64)p.rate_off * dt, 0xffffffffull);
    if (c[0] < p_on) off_on = (unsigned)(((u64)c[2] * dt) >> 32);
    if (c[1] < p_off) off_off = (unsigned)(((u64)c[3] * dt) >> 32);
}

// The candidates of a pixel at one frame.
struct ef_cands {
    unsigned m;               // signal: m crossings of polarity `on` at the levels r0 +- j * c
    bool on;
    int r0, c;
    int a_level, lev;         // L[k-1], L[k]
    int64_t t_prev, t_k;      // T[k-1], T[k]
    bool same;                // every candidate is stamped t_k (frame stamps, or frame 0 of the call)
    unsigned off_on, off_off; // noise: offsets from t_prev, EF_NONE for none
};

// The linear stamp of the crossing of `level` on the way from a_level at t_prev to lev at t_k (no way at all: t_k).
__device__ __forceinline__ int64_t ef_stamp(long long level, int a_level, int lev, int64_t t_prev, int64_t t_k)
{
    const long long span = (long long)lev - (long long)a_level, off = level - (long long)a_level;
    const u64 den = (u64)(span < 0 ? -span : span);
    return den ? t_prev + (int64_t)(((u64)(off < 0 ? -off : off) * (u64)(t_k - t_prev)) / den) : t_k;
}

// The candidates of frame k from its level: r and prev_level (L[k - 1]) move on.  A frame past the last has none and moves
// nothing.  Without SENSOR there are no times and no noise: the crossings alone.
template <int SENSOR>
__device__ __forceinline__ void ef_frame(const ef_args& a, const ef_sensor& s, ef_px& q, const ef_spx& p, int k, int lev, bool linear,
                                         int& prev_level, ef_cands& c)
{
    c.m = 0;
    c.on = false;
    c.same = true;
    c.off_on = c.off_off = EF_NONE;
    if (k >= a.n) return;
    c.lev = lev;
    c.a_level = prev_level;
    prev_level = lev;
    c.r0 = q.r;
    c.m = ef_step(q.r, lev, q.c_on, q.c_off, c.on);
    c.c = c.on ? q.c_on : q.c_off;
    if constexpr (SENSOR) {
        c.t_k = a.times[k];
        c.t_prev = a.times[max(k - 1, 0)];
        c.same = !linear || k == 0;
        if (s.noise && k > 0) ef_noise(s, q, p, k, (u64)(c.t_k - c.t_prev), c.off_on, c.off_off);
    }
}

// The refractory walk of one frame: the candidates in the order (t, signal before ON noise before OFF noise), a candidate
// emitted iff t >= t_ok, and then t_ok = t + refractory.  emit(kind, count, t): kind 0 = `count` signal crossings in a row
// (the next ones of the pixel's order), 1 = the ON noise event, 2 = the OFF noise event.  With one stamp for all the walk
// is closed: nothing if t_k < t_ok, the first candidate alone under a refractory time, else all of them.
template <int LINEAR, class Emit>
__device__ __forceinline__ void ef_walk(const ef_cands& c, long long refractory, int64_t& t_ok, Emit&& emit)
{
    const bool has_on = c.off_on != EF_NONE, has_off = c.off_off != EF_NONE;
    if (!LINEAR || c.same) {
        if (!(c.m || has_on || has_off) || c.t_k < t_ok) return;
        if (refractory > 0) {
            emit(c.m ? 0 : has_on ? 1 : 2, 1u, c.t_k);
        } else {
            if (c.m) emit(0, c.m, c.t_k);
            if (has_on) emit(1, 1u, c.t_k);
            if (has_off) emit(2, 1u, c.t_k);
        }
        t_ok = (int64_t)((u64)c.t_k + (u64)refractory);
        return;
    }
    // the (at most two) noise candidates in time order, ON first on a tie
    int nn = (int)has_on + (int)has_off;
    int64_t tn0 = c.t_prev + (int64_t)c.off_on, tn1 = c.t_prev + (int64_t)c.off_off;
    int kn0 = 1, kn1 = 2;
    if (!has_on || (has_off && tn1 < tn0)) {
        const int64_t t = tn0;
        tn0 = tn1;
        tn1 = t;
        kn0 = 2;
        kn1 = 1;
    }
    long long level = c.r0;
    for (unsigned i = 0; i < c.m; i++) {
        level += c.on ? c.c : -c.c;
        const int64_t t = ef_stamp(level, c.a_level, c.lev, c.t_prev, c.t_k);
        while (nn && tn0 < t) {   // noise strictly before this crossing: a signal crossing goes first on a tie
            if (tn0 >= t_ok) {
                t_ok = (int64_t)((u64)tn0 + (u64)refractory);
                emit(kn0, 1u, tn0);
            }
            tn0 = tn1;
            kn0 = kn1;
            nn--;
        }
        if (t >= t_ok) {
            t_ok = (int64_t)((u64)t + (u64)refractory);
            emit(0, 1u, t);
        }
    }
    while (nn) {
        if (tn0 >= t_ok) {
            t_ok = (int64_t)((u64)tn0 + (u64)refractory);
            emit(kn0, 1u, tn0);
        }
        tn0 = tn1;
        kn0 = kn1;
        nn--;
    }
}

// The events of a pixel at frame k that survive, per polarity; t_ok moves on.  Without a walk (nothing can be dropped:
// always so without SENSOR) they are the candidates and t_ok is left alone.
template <int LINEAR, int SENSOR>
__device__ __forceinline__ void ef_survivors(const ef_sensor& s, const ef_cands& c, int64_t& t_ok, unsigned& n_on, unsigned& n_off)
{
    n_on = n_off = 0;
    if (!SENSOR || !s.walk) {
        n_on = (c.on ? c.m : 0u) + (c.off_on != EF_NONE);
        n_off = (c.on ? 0u : c.m) + (c.off_off != EF_NONE);
        return;
    }
    ef_walk<LINEAR>(c, s.refractory, t_ok, [&](int kind, unsigned count, int64_t) {
        const bool to_on = kind == 0 ? c.on : kind == 1;   // (no branch: the two sums stay in registers)
        n_on += to_on ? count : 0u;
        n_off += to_on ? 0u : count;
    });
}

// bad[0]: a threshold plane holds a value < 1; bad[1]: a step of EF_WALK_MAX crossings or more under a walk (SENSOR).
template <int SENSOR>
__global__ __launch_bounds__(EF_WG) void k_ef_count(ef_args a, ef_sensor s, u64* __restrict__ table, u64* __restrict__ bad)
{
    __shared__ int sh_lut[256];
    __shared__ u64 sh[2][EF_BATCH][2][4];   // [set][frame of the batch][polarity][wave]; two sets used in turn: one barrier per batch
    ef_px q = ef_init(a, sh_lut);
    if (q.in && (q.c_on < 1 || q.c_off < 1)) *bad = 1;
    ef_spx sp{};
    int prev_level = 0;   // L[k - 1]
    if (SENSOR) sp = ef_sensor_init(s, q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n_wg = gridDim.x;
    int set = 0;
    for (int k0 = 0; k0 < a.n; k0 += EF_BATCH, set ^= 1) {
        unsigned f[EF_BATCH];
        ef_load(a, q, k0, f);
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            ef_cands c;
            ef_frame<SENSOR>(a, s, q, sp, k0 + j, sh_lut[f[j]], s.linear, prev_level, c);
            if (SENSOR && s.walk && !c.same && c.m >= EF_WALK_MAX) {
                if (q.in) bad[1] = 1;
                c.m = 0;   // the call is refused: no long walk for nothing
            }
            unsigned n_on, n_off;   // the pixel's events of the frame
            ef_survivors<1, SENSOR>(s, c, sp.t_ok, n_on, n_off);   // (the stamp mode of the count pass is c.same)
            if (!q.in) n_on = n_off = 0;
            u64 s_on, s_off;
            if (!__any((n_on | n_off) >> 24)) {   // every lane below 2^24 (any frame of the linear table): the wave's sums fit 32 bits
                s_on = ev_wave_last(ev_wave_scan(n_on));
                s_off = ev_wave_last(ev_wave_scan(n_off));
            } else {
                s_on = n_on;
                s_off = n_off;
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

// meta: [0 .. 2n) the bases of the (frame, polarity) rows, [2n] the total, [2n + 1] the bad-threshold flag, [2n + 2] the
// long-walk flag (which the plain kernels never raise).  The emit and unpack kernels write only under ev_guard(meta + 2n).

// Where the emit pass writes.
struct ef_out {
    int p_on, p_off;
    int16_t *x, *y;           // frame stamps: the caller's arrays
    int8_t* p;
    int64_t* t;
    u64* keys;                // linear stamps: (t - T[0], (x, y, polarity)) pairs for the reorder
    unsigned* vals;
    int32_t* ref;
    int64_t* t_ok;            // SENSOR
};

// Event `at` of the emitted order: the pixel's, of polarity `on` (pv: its byte, chosen by the caller -- a select between
// o.p_on and o.p_off in here put both on the stack), stamped t.
template <int LINEAR>
__device__ __forceinline__ void ef_store(const ef_out& o, size_t at, const ef_px& q, bool on, int8_t pv, int64_t t, int64_t t_first)
{
    if (LINEAR) {
        o.keys[at] = (u64)(t - t_first);
        o.vals[at] = (unsigned)q.x | ((unsigned)q.y << 15) | (on ? 1u << 30 : 0u);
    } else {
        o.x[at] = (int16_t)q.x;
        o.y[at] = (int16_t)q.y;
        o.p[at] = pv;
        o.t[at] = t;
    }
}

// Where the workgroup's ON and OFF events of the frames k0 .. k0 + EF_BATCH - 1 start (the same in every lane).
__device__ __forceinline__ void ef_bases(const ef_args& a, const u64* __restrict__ table, const u64* __restrict__ meta, int k0,
                                         u64 (&base)[EF_BATCH][2])
{
#pragma unroll
    for (int j = 0; j < EF_BATCH; j++) {
        const size_t row = (size_t)min(k0 + j, a.n - 1) * 2;
        base[j][0] = meta[row] + table[row * gridDim.x + blockIdx.x];
        base[j][1] = meta[row + 1] + table[(row + 1) * gridDim.x + blockIdx.x];
    }
}

// The plain emit pass (k_ef_emit<LINEAR, 0>).
template <int LINEAR>
__device__ __forceinline__ void ef_emit_plain(const ef_args& a, const u64* __restrict__ table, const u64* __restrict__ meta, const ef_out& o)
{
    __shared__ int sh_lut[256];
    __shared__ unsigned sh[2][EF_BATCH][2][4];
    ef_px q = ef_init(a, sh_lut);
    const int64_t t_first = a.times[0];
    int prev_level = 0;   // L[k - 1]
    int set = 0;
    for (int k0 = 0; k0 < a.n; k0 += EF_BATCH, set ^= 1) {
        unsigned f[EF_BATCH];
        ef_load(a, q, k0, f);
        unsigned m[EF_BATCH], excl[EF_BATCH];
        int r0[EF_BATCH], lev[EF_BATCH];
        bool on[EF_BATCH];
        u64 base[EF_BATCH][2];
        ef_bases(a, table, meta, k0, base);
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            lev[j] = sh_lut[f[j]];
            r0[j] = q.r;
            on[j] = false;
            m[j] = 0;
            if (k0 + j < a.n) m[j] = ef_step(q.r, lev[j], q.c_on, q.c_off, on[j]);
            if (!q.in) m[j] = 0;
            // the total is below 2^31 (the guard), so 32 bits hold every prefix
            const unsigned i_on = ev_wave_scan(on[j] ? m[j] : 0u), i_off = ev_wave_scan(on[j] ? 0u : m[j]);
            ev_wg_put(sh[set][j][0], i_on);
            ev_wg_put(sh[set][j][1], i_off);
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
            const unsigned before = ev_wg_collect(sh[set][j][pol]).before;
            if (m[j] == 0) continue;
            size_t at = (size_t)(on[j] ? base[j][0] : base[j][1]) + before + excl[j];
            const int64_t t_k = a.times[k];
            const bool linear = LINEAR && k > 0;
            const int64_t t_prev = linear ? a.times[k - 1] : t_k;
            const int c = on[j] ? q.c_on : q.c_off;
            const int8_t pv = (int8_t)(on[j] ? o.p_on : o.p_off);
            long long level = r0[j];
            for (unsigned i = 0; i < m[j]; i++, at++) {
                level += on[j] ? c : -c;
                ef_store<LINEAR>(o, at, q, on[j], pv, linear ? ef_stamp(level, a_level, lev[j], t_prev, t_k) : t_k, t_first);
            }
        }
    }
    if (q.in && o.ref) o.ref[q.pix] = q.r;
}

// The emit pass of the sensor model (k_ef_emit<LINEAR, 1>).  A pixel may have events of both polarities at one frame (a
// signal step and noise), so both prefixes are kept.  Each frame is walked twice, from two copies of t_ok that move alike:
// before the barrier for the counts the prefixes need, after it to write.  A noise event is the last of its polarity.
template <int LINEAR>
__device__ __forceinline__ void ef_emit_sensor(const ef_args& a, const ef_sensor& s, const u64* __restrict__ table,
                                               const u64* __restrict__ meta, const ef_out& o)
{
    __shared__ int sh_lut[256];
    __shared__ unsigned sh[2][EF_BATCH][2][4];
    ef_px q = ef_init(a, sh_lut);
    ef_spx sp = ef_sensor_init(s, q);
    int64_t t_ok = sp.t_ok;   // the writing walk's copy; sp.t_ok is the counting walk's
    const int64_t t_first = a.times[0];
    int prev_level = 0;   // L[k - 1]
    int set = 0;
    for (int k0 = 0; k0 < a.n; k0 += EF_BATCH, set ^= 1) {
        unsigned f[EF_BATCH];
        ef_load(a, q, k0, f);
        ef_cands c[EF_BATCH];
        unsigned incl[EF_BATCH][2], cnt[EF_BATCH][2];
        u64 base[EF_BATCH][2];
        ef_bases(a, table, meta, k0, base);
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            ef_frame<1>(a, s, q, sp, k0 + j, sh_lut[f[j]], LINEAR, prev_level, c[j]);
            ef_survivors<LINEAR, 1>(s, c[j], sp.t_ok, cnt[j][0], cnt[j][1]);
            if (!q.in) cnt[j][0] = cnt[j][1] = 0;
            // the total is below 2^31 (the guard), so 32 bits hold every prefix
            incl[j][0] = ev_wave_scan(cnt[j][0]);
            incl[j][1] = ev_wave_scan(cnt[j][1]);
            ev_wg_put(sh[set][j][0], incl[j][0]);
            ev_wg_put(sh[set][j][1], incl[j][1]);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < EF_BATCH; j++) {
            if (k0 + j >= a.n) break;
            const unsigned before[2] = {ev_wg_collect(sh[set][j][0]).before, ev_wg_collect(sh[set][j][1]).before};
            if (!q.in || (c[j].m == 0 && c[j].off_on == EF_NONE && c[j].off_off == EF_NONE)) continue;
            // the pixel's ON events are [end_on - cnt, end_on), its OFF events likewise
            const size_t end_on = (size_t)base[j][0] + before[0] + incl[j][0], end_off = (size_t)base[j][1] + before[1] + incl[j][1];
            size_t at = c[j].on ? end_on - cnt[j][0] : end_off - cnt[j][1];   // the next signal event
            const bool sig_on = c[j].on;
            // (the polarity bytes are captured by value: chosen between through two references they went to the stack)
            ef_walk<LINEAR>(c[j], s.refractory, t_ok, [&, p_on = o.p_on, p_off = o.p_off](int kind, unsigned count, int64_t t) {
                const bool is_on = kind == 0 ? sig_on : kind == 1;
                size_t w = kind == 0 ? at : kind == 1 ? end_on - 1 : end_off - 1;
                at += kind == 0 ? count : 0u;
                for (unsigned i = 0; i < count; i++, w++) ef_store<LINEAR>(o, w, q, is_on, (int8_t)(is_on ? p_on : p_off), t, t_first);
            });
        }
    }
    if (q.in && o.ref) o.ref[q.pix] = q.r;
    if (q.in && o.t_ok) o.t_ok[q.pix] = t_ok;
}

template <int LINEAR, int SENSOR>
__global__ __launch_bounds__(EF_WG) void k_ef_emit(ef_args a, ef_sensor s, const u64* __restrict__ table, const u64* __restrict__ meta,
                                                   u64 expected, ef_out o)
{
    if (!ev_guard(meta + 2 * (size_t)a.n, expected)) return;
    if constexpr (SENSOR)
        ef_emit_sensor<LINEAR>(a, s, table, meta, o);
    else
        ef_emit_plain<LINEAR>(a, table, meta, o);
}

__global__ __launch_bounds__(EF_WG) void k_ef_unpack(size_t count, const u64* __restrict__ keys, const unsigned* __restrict__ vals,
                                                     const u64* __restrict__ meta, int n, u64 expected, int64_t t_first, int p_on,
                                                     int p_off, int16_t* __restrict__ ox, int16_t* __restrict__ oy,
                                                     int8_t* __restrict__ op, int64_t* __restrict__ ot)
{
    if (!ev_guard(meta + 2 * (size_t)n, expected)) return;
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
    int mode;                         // the stamp mode (the count entry of the plain pair: unused)
    const nsof_events_sensor* sensor; // nullptr: the plain generator
};

// Every refusal of the arguments both entries share; nothing launched.
int ef_check(nsof_ctx* ctx, const char* who, const ef_call& c)
{
    if (c.n < 1 || c.H < 1 || c.W < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: %d frames of %dx%d", who, c.n, c.W, c.H);
    if (!ev_sensor_ok(c.H, c.W))
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
    if (c.mode != NSOF_EVENTS_T_FRAME && c.mode != NSOF_EVENTS_T_LINEAR)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: timestamps_mode %d", who, c.mode);
    if (const nsof_events_sensor* s = c.sensor) {
        if (s->refractory_us < 0 || s->refractory_us >= (1ll << 31))
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: refractory_us = %lld is outside [0, 2^31)", who, (long long)s->refractory_us);
        if (s->first_frame < 0 || s->first_frame > (1ll << 62) - c.n)
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: first_frame = %lld with %d frames: frame indices lie in [0, 2^62]", who,
                                  (long long)s->first_frame, c.n);
        // t_ok = t + refractory_us of the latest stamp there can be must stay an int64: wrapped, the pixel would never be blocked again
        if (s->refractory_us > 0 && c.times[c.n - 1] > INT64_MAX - s->refractory_us)
            return nsof_set_error(ctx, NSOF_EINVAL, "%s: times[%d] = %lld with refractory_us = %lld: t_ok = t + refractory_us would "
                                  "pass the int64 range", who, c.n - 1, (long long)c.times[c.n - 1], (long long)s->refractory_us);
    }
    return NSOF_OK;
}

// The sensor arguments as the kernels take them (all zero for the plain generator, whose kernels leave them alone).
ef_sensor ef_sensor_args(const ef_call& c)
{
    ef_sensor d{};
    if (const nsof_events_sensor* s = c.sensor) {
        d.refractory = s->refractory_us;
        d.first_frame = s->first_frame;
        d.k0 = (unsigned)s->seed;
        d.k1 = (unsigned)(s->seed >> 32);
        d.rate_on = s->rate_on_q;
        d.rate_off = s->rate_off_q;
        d.rate_plane = s->d_rate_plane;
        d.t_ok_in = s->d_t_ok_in;
        d.noise = s->d_rate_plane || s->rate_on_q || s->rate_off_q;
        d.walk = s->refractory_us > 0 || s->d_t_ok_in;
        d.linear = c.mode == NSOF_EVENTS_T_LINEAR;
    }
    return d;
}

// The workspace of a call, carved from ctx->tmp in one reservation.
struct ef_plan {
    ef_args args;
    size_t n_wg;
    ef_sensor sensor;
    u64 *table, *meta;        // [2n][n_wg]; [2n + 3]
    u64 *keys_in, *keys_out;  // linear time stamps: [count] each
    unsigned *vals_in, *vals_out;
    void* sort_tmp;
    size_t sort_bytes;
};

// The count and the emit launch: the instantiation picked, then launched on one workgroup per 256 pixels.
void ef_launch_count(hipStream_t stream, const ef_plan& pl, bool sensor)
{
    const auto kernel = sensor ? k_ef_count<1> : k_ef_count<0>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.n_wg), dim3(EF_WG), 0, stream, pl.args, pl.sensor, pl.table, pl.meta + 2 * (size_t)pl.args.n + 1);
}

void ef_launch_emit(hipStream_t stream, const ef_plan& pl, bool linear, bool sensor, u64 total, const ef_out& o)
{
    const auto kernel = sensor ? (linear ? k_ef_emit<1, 1> : k_ef_emit<0, 1>) : (linear ? k_ef_emit<1, 0> : k_ef_emit<0, 0>);
    hipLaunchKernelGGL(kernel, dim3((unsigned)pl.n_wg), dim3(EF_WG), 0, stream, pl.args, pl.sensor, pl.table, pl.meta, total, o);
}

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
    pl->sort_bytes = 0;
    if (sort_count)
        NSOF_HIP(ctx, rocprim::radix_sort_pairs(nullptr, pl->sort_bytes, (const u64*)nullptr, (u64*)nullptr, (const unsigned*)nullptr,
                                                (unsigned*)nullptr, sort_count, 0u, ef_key_bits(c), ctx->stream));
    ev_carve w;   // (sort_count == 0: the buffers of the reorder are empty and take nothing)
    const size_t o_table = w.take(rows * pl->n_wg * sizeof(u64)), o_meta = w.take((rows + 3) * sizeof(u64));
    const size_t o_keys = w.take(sort_count * sizeof(u64)), o_keys_out = w.take(sort_count * sizeof(u64));
    const size_t o_vals = w.take(sort_count * sizeof(unsigned)), o_vals_out = w.take(sort_count * sizeof(unsigned)), o_sort = w.at;
    if (int rc = ctx->tmp.reserve(ctx, o_sort + pl->sort_bytes)) return rc;
    char* ws = (char*)ctx->tmp.p;
    pl->table = (u64*)(ws + o_table);
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

    pl->sensor = ef_sensor_args(c);
    NSOF_HIP(ctx, hipMemsetAsync(pl->meta + rows + 1, 0, 2 * sizeof(u64), ctx->stream));   // the bad-threshold and long-walk flags
    ef_launch_count(ctx->stream, *pl, c.sensor != nullptr);
    NSOF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ev_scan<true>, dim3((unsigned)rows), dim3(EF_WG), 0, ctx->stream, pl->table, pl->n_wg, pl->meta);
    NSOF_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ev_scan<true>, dim3(1), dim3(EF_WG), 0, ctx->stream, pl->meta, rows, pl->meta + rows);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// The count entry of both pairs.
int ef_count_entry(nsof_ctx* ctx, const char* who, const ef_call& c, int64_t* frame_bounds_out)
{
    if (int rc = ef_check(ctx, who, c)) return rc;
    if (!frame_bounds_out) return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (frame_bounds_out)", who);
    ef_plan pl;
    if (int rc = ef_count_pass(ctx, c, 0, &pl)) return rc;
    const int n = c.n;
    const size_t rows = 2 * (size_t)n;
    std::vector<u64> meta(rows + 3);
    NSOF_HIP(ctx, hipMemcpyAsync(meta.data(), pl.meta, meta.size() * sizeof(u64), hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (meta[rows + 1])
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: the threshold plane holds a value < 1", who);
    if (meta[rows + 2])
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%s: a pixel crosses 2^20 thresholds or more in one step, beyond the refractory walk "
                              "of linear time stamps", who);
    if (meta[rows] >= (u64)EV_MAX_EVENTS)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%s: %llu%s events, 2^31 or more", who, meta[rows], meta[rows] == ~0ull ? " or more" : "");
    for (int k = 0; k < n; k++) frame_bounds_out[k] = (int64_t)meta[2 * (size_t)k];
    frame_bounds_out[n] = (int64_t)meta[rows];
    return NSOF_OK;
}

// The emit entry of both pairs.
int ef_emit_entry(nsof_ctx* ctx, const char* who, const ef_call& c, const int64_t* frame_bounds, int p_on, int p_off, int64_t capacity,
                  int16_t* d_x, int16_t* d_y, int8_t* d_p, int64_t* d_t, int32_t* d_ref_out, int64_t* d_t_ok_out)
{
    if (int rc = ef_check(ctx, who, c)) return rc;
    const int n = c.n;
    if (!frame_bounds) return nsof_set_error(ctx, NSOF_EINVAL, "%s: null pointer (frame_bounds)", who);
    if (p_on < -128 || p_on > 127 || p_off < -128 || p_off > 127)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: p_on = %d, p_off = %d do not fit an int8", who, p_on, p_off);
    const int64_t total = frame_bounds[n];
    if (total < 0 || total >= EV_MAX_EVENTS)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: frame_bounds[%d] = %lld is not a total the count entry gives", who, n, (long long)total);
    if (capacity < total)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: capacity %lld is below the %lld events of the stream", who, (long long)capacity,
                              (long long)total);
    if (total > 0)
        if (int rc = ev_check_stream(ctx, who, d_x, d_y, d_p, d_t)) return rc;
    if (c.sensor && c.sensor->d_t_ok_in && !d_t_ok_out)
        return nsof_set_error(ctx, NSOF_EINVAL, "%s: d_t_ok_in without d_t_ok_out: the run could not be continued", who);
    const bool linear = c.mode == NSOF_EVENTS_T_LINEAR && total > 0;
    ef_plan pl;
    if (int rc = ef_count_pass(ctx, c, linear ? (size_t)total : 0, &pl)) return rc;
    const ef_out o{p_on, p_off, d_x, d_y, d_p, d_t, pl.keys_in, pl.vals_in, d_ref_out, d_t_ok_out};
    // (an empty linear stream has no pairs to sort, but the sensor kernel still takes its stamp mode: ref and t_ok)
    ef_launch_emit(ctx->stream, pl, c.sensor ? c.mode == NSOF_EVENTS_T_LINEAR : linear, c.sensor != nullptr, (u64)total, o);
    NSOF_HIP(ctx, hipGetLastError());
    if (linear) {
        NSOF_HIP(ctx, rocprim::radix_sort_pairs(pl.sort_tmp, pl.sort_bytes, (const u64*)pl.keys_in, pl.keys_out, (const unsigned*)pl.vals_in,
                                                pl.vals_out, (size_t)total, 0u, ef_key_bits(c), ctx->stream));
        hipLaunchKernelGGL(k_ef_unpack, dim3((unsigned)(((size_t)total + EF_WG - 1) / EF_WG)), dim3(EF_WG), 0, ctx->stream, (size_t)total,
                           pl.keys_out, pl.vals_out, pl.meta, n, (u64)total, c.times[0], p_on, p_off, d_x, d_y, d_p, d_t);
        NSOF_HIP(ctx, hipGetLastError());
    }
    return NSOF_OK;
}

}  // namespace

extern "C" int nsof_events_from_frames_count_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                                 int n, int height, int width, const int64_t* times, const int32_t* lut, int c_on,
                                                 int c_off, const int32_t* d_thr_plane, const int32_t* d_ref_in, int ref_mode,
                                                 int64_t* frame_bounds_out)
{
    if (!ctx) return NSOF_EINVAL;
    const ef_call c{d_frames, row_stride, frame_stride, n, height, width, times, lut, c_on, c_off, d_thr_plane, d_ref_in, ref_mode,
                    NSOF_EVENTS_T_FRAME, nullptr};
    return ef_count_entry(ctx, "events_from_frames_count", c, frame_bounds_out);
}

extern "C" int nsof_events_from_frames_emit_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                                int n, int height, int width, const int64_t* times, const int32_t* lut, int c_on,
                                                int c_off, const int32_t* d_thr_plane, const int32_t* d_ref_in, int ref_mode,
                                                const int64_t* frame_bounds, int timestamps_mode, int p_on, int p_off,
                                                int64_t capacity, int16_t* d_x, int16_t* d_y, int8_t* d_p, int64_t* d_t,
                                                int32_t* d_ref_out)
{
    if (!ctx) return NSOF_EINVAL;
    const ef_call c{d_frames, row_stride, frame_stride, n, height, width, times, lut, c_on, c_off, d_thr_plane, d_ref_in, ref_mode,
                    timestamps_mode, nullptr};
    return ef_emit_entry(ctx, "events_from_frames_emit", c, frame_bounds, p_on, p_off, capacity, d_x, d_y, d_p, d_t, d_ref_out, nullptr);
}

extern "C" int nsof_events_from_frames_sensor_count_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride,
                                                        ptrdiff_t frame_stride, int n, int height, int width, const int64_t* times,
                                                        const int32_t* lut, int c_on, int c_off, const int32_t* d_thr_plane,
                                                        const int32_t* d_ref_in, int ref_mode, int timestamps_mode,
                                                        const nsof_events_sensor* sensor, int64_t* frame_bounds_out)
{
    if (!ctx) return NSOF_EINVAL;
    const ef_call c{d_frames, row_stride, frame_stride, n, height, width, times, lut, c_on, c_off, d_thr_plane, d_ref_in, ref_mode,
                    timestamps_mode, sensor};
    return ef_count_entry(ctx, "events_from_frames_sensor_count", c, frame_bounds_out);
}

extern "C" int nsof_events_from_frames_sensor_emit_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride,
                                                       ptrdiff_t frame_stride, int n, int height, int width, const int64_t* times,
                                                       const int32_t* lut, int c_on, int c_off, const int32_t* d_thr_plane,
                                                       const int32_t* d_ref_in, int ref_mode, const int64_t* frame_bounds,
                                                       int timestamps_mode, int p_on, int p_off, int64_t capacity, int16_t* d_x,
                                                       int16_t* d_y, int8_t* d_p, int64_t* d_t, int32_t* d_ref_out,
                                                       const nsof_events_sensor* sensor, int64_t* d_t_ok_out)
{
    if (!ctx) return NSOF_EINVAL;
    const ef_call c{d_frames, row_stride, frame_stride, n, height, width, times, lut, c_on, c_off, d_thr_plane, d_ref_in, ref_mode,
                    timestamps_mode, sensor};
    return ef_emit_entry(ctx, "events_from_frames_sensor_emit", c, frame_bounds, p_on, p_off, capacity, d_x, d_y, d_p, d_t, d_ref_out,
                         d_t_ok_out);
}

extern "C" void nsof_events_noise_draw(uint64_t seed, uint32_t pixel, int64_t frame, uint32_t* out)
{
    unsigned c[4] = {pixel, (unsigned)(uint64_t)frame, (unsigned)((uint64_t)frame >> 32), EF_NOISE_WORD};
    philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
    for (int i = 0; i < 4; i++) out[i] = c[i];
}
