// ROI gating on the device: the reference thresholds a tiny map of device currents, labels its
// 4-connected components and turns their bounding boxes into crop rectangles
// (/root/reference/optical_flow_seg.py:115-121 update_transition_pic, :211-252 opticalFlow3D, :426-431 current -> gray).
// A map of up to 64 x 64 cells (the reference's are 4 x 4 .. 13 x 24) is owned by ONE wavefront (k_roi_gate); larger
// maps, up to 2^27 cells, take the union-find launches further down (k_ccl_*), with the same results.  k_roi_gate:
//   lane r      holds row r of the thresholded map as a 64-bit mask (bit c = column c);
//   components  are taken in raster order of their first cell (the label order of cv2.connectedComponentsWithStats and
//               of the host mirror nsof_roi_from_surface): seed = first set bit of the first non-empty row, then a flood
//               fill by mask arithmetic -- S |= (S << 1 | S >> 1 | S of the row above | S of the row below) & R, the
//               neighbouring rows through wave shuffles -- until no lane changes (a ballot);
//   boxes       top / bottom from a ballot of the non-empty rows, left / right from the OR of all rows (xor-shuffle
//               reduction); scaled by MEMSIZE, extended and clipped exactly as the reference does.
// Output per map: the number of rectangles and rects[cap][4] = (x0, y0, x1, y1), FLAG 1 one per component, FLAG 2 their union.
#include <algorithm>
#include <climits>
#include <cmath>

#include "nsof_internal.h"

namespace {

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// The 8-bit gating value of a device current (optical_flow_seg.py:426-431): every gating kernel's one expression.
__device__ __forceinline__ int gate_gray(double current)
{
    double g = -3366.0 / log10(current) - 306.0;
    g = g < 0.0 ? 0.0 : (g > 255.0 ? 255.0 : g);        // NaN (I <= 0) compares false twice and casts to 0
    return (g == g) ? (int)(unsigned char)g : 0;
}

__global__ __launch_bounds__(64) void k_roi_gate(const double* __restrict__ cur, size_t map_stride, int rows, int cols, int fw,
                                                 int fh, int ms, int thres, int el, int er, int eu, int ed, int conn8, int flag,
                                                 int cap, int* __restrict__ counts, int* __restrict__ rects,
                                                 unsigned char* __restrict__ gray)
{
    const int k = blockIdx.x, lane = threadIdx.x;
    const double* m = cur + (size_t)k * map_stride;
    unsigned long long R = 0;
    if (lane < rows) {
        for (int c = 0; c < cols; c++) {
            const int gi = gate_gray(m[(size_t)lane * cols + c]);
            if (gray) gray[((size_t)k * rows + lane) * cols + c] = (unsigned char)gi;
            if (gi >= thres) R |= 1ull << c;
        }
    }
    int* out = rects + (size_t)k * cap * 4;
    int n = 0, ux0 = 1 << 30, uy0 = 1 << 30, ux1 = -1, uy1 = -1;
    auto emit = [&](int bx0, int by0, int bx1, int by1) {   // cell box (inclusive) -> frame rectangle
        if (lane == 0 && n < cap) {
            out[4 * n] = max(bx0 * ms - el, 0);
            out[4 * n + 1] = max(by0 * ms - eu, 0);
            out[4 * n + 2] = min((bx1 + 1) * ms + er, fw);
            out[4 * n + 3] = min((by1 + 1) * ms + ed, fh);
        }
        n++;
    };
    for (int guard = 0; guard < 64 * 64; guard++) {   // at most one component per cell
        const unsigned long long any = __ballot(R != 0);
        if (!any) break;
        const int r0 = __ffsll((long long)any) - 1;
        const unsigned long long Rr0 = __shfl(R, r0);
        const int c0 = __ffsll((long long)Rr0) - 1;
        unsigned long long S = lane == r0 ? (1ull << c0) : 0;
        for (int it = 0; it < 64 * 64; it++) {
            unsigned long long up = __shfl_up(S, 1), dn = __shfl_down(S, 1);
            if (lane == 0) up = 0;
            if (lane == 63) dn = 0;
            unsigned long long N = S | (S << 1) | (S >> 1) | up | dn;
            if (conn8) N |= (up << 1) | (up >> 1) | (dn << 1) | (dn >> 1);
            N &= R;
            if (!__ballot(N != S)) break;
            S = N;
        }
        const unsigned long long rmask = __ballot(S != 0), cmask = wave_or(S);
        const int by0 = __ffsll((long long)rmask) - 1, by1 = 63 - __clzll((long long)rmask);
        const int bx0 = __ffsll((long long)cmask) - 1, bx1 = 63 - __clzll((long long)cmask);
        if (flag == 1) {
            emit(bx0, by0, bx1, by1);
        } else {
            ux0 = min(ux0, bx0); uy0 = min(uy0, by0); ux1 = max(ux1, bx1); uy1 = max(uy1, by1);
        }
        R &= ~S;
    }
    if (flag == 2 && ux1 >= 0) emit(ux0, uy0, ux1, uy1);
    if (lane == 0) counts[k] = n;
}

// ---- maps above 64 x 64 cells: union-find over a parent array in the workspace -----------------------------------
// Every launch below covers a chunk of maps with CCL_TILE consecutive raster cells per workgroup (tile t of map m is
// workgroup m * ntile + t).  parent[i] of a map: -1 for an OFF cell; for an ON cell an ON cell of the same component
// with parent[i] <= i, so every link points from the larger raster index to the smaller and the root of a component
// is its first cell in raster order -- the label order of cv2 and of the host mirror, whatever the scheduling.
//   k_ccl_init     gray map, ON bits; parent = the head of the cell's horizontal run inside its tile (an LDS scan)
//                  FLAG 2 needs no labels: the union box is the box of all ON cells (wave min / max, agent atomics)
//   k_ccl_merge    each ON cell unions with the earlier neighbours its run does not already reach (left across a tile
//                  edge, up; up-left / up-right with 8-connectivity): lock-free, agent-scope atomic loads and atomic min
//   k_ccl_flatten  each ON cell finds its root and points at it; the number of roots per tile
//   k_ccl_scan     per map: exclusive scan of the tiles' root counts = the true component count; resets the boxes
//   k_ccl_label    each root's slot becomes -2 - (its rank in raster order)
//   k_ccl_stats    cell boxes of the components with label < cap (one agent atomic per label per wave)
//   k_ccl_emit     cell boxes -> frame rectangles, exactly as k_roi_gate scales, extends and clips them
// Data crosses workgroups only at launch boundaries or through agent-scope atomics; no loop waits on another workgroup.
constexpr int CCL_TILE = 256;

__device__ __forceinline__ int ccl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ccl_min(int* p, int v) { __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ccl_min_ret(int* p, int v)
{
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of ON cell x, halving the path on the way (atomic min: the grandparent is an ancestor too).  A parent is always
// smaller than its cell, so the walk ends within x + 1 steps; a stale read only returns an older ancestor.
__device__ int ccl_find(int* par, int x)
{
    for (int guard = x; guard >= 0; guard--) {
        const int p = ccl_load(par + x);
        if (p == x) break;
        const int gp = ccl_load(par + p);
        if (gp < p) ccl_min(par + x, gp);
        x = gp;
    }
    return x;
}

// Join the components of ON cells a and b: the larger root is linked to the smaller by an atomic min.  If the min finds
// that root already linked elsewhere, the link it replaced is joined next; the larger of the two indices in hand drops
// on every pass, so the loop ends within max(a, b) + 1 passes.
__device__ void ccl_union(int* par, int a, int b)
{
    for (int guard = a > b ? a : b; guard >= 0; guard--) {
        a = ccl_find(par, a);
        b = ccl_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = ccl_min_ret(par + a, b);
        if (old == a) return;
        a = old;
    }
}

__device__ __forceinline__ int wave_min_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ int wave_max_i(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// Cell box (x0, y0, x1, y1) of the lanes with `mine` set, folded into box[0..3] by one lane (`leader`).  CHECK: the box
// only grows, so a bound that an atomic load shows already reached needs no atomic -- for FLAG 2's one box per map, which
// every wave of the map would otherwise hit with the same four atomics; the labels' boxes take the atomics unchecked.
template <bool CHECK>
__device__ __forceinline__ void ccl_box_fold(bool mine, int leader, int x, int y, int* box)
{
    const int x0 = wave_min_i(mine ? x : INT_MAX), y0 = wave_min_i(mine ? y : INT_MAX);
    const int x1 = wave_max_i(mine ? x : -1), y1 = wave_max_i(mine ? y : -1);
    if ((int)__lane_id() == leader) {
        if (!CHECK || ccl_load(box) > x0) ccl_min(box, x0);
        if (!CHECK || ccl_load(box + 1) > y0) ccl_min(box + 1, y0);
        if (!CHECK || ccl_load(box + 2) < x1) __hip_atomic_fetch_max(box + 2, x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!CHECK || ccl_load(box + 3) < y1) __hip_atomic_fetch_max(box + 3, y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ void ccl_box_reset(int* box)
{
    box[0] = INT_MAX; box[1] = INT_MAX; box[2] = -1; box[3] = -1;
}

// FLAG 2: the union box of map k starts empty (rects[k][0]).
__global__ __launch_bounds__(CCL_TILE) void k_ccl_box_reset(int n_maps, int* __restrict__ rects, int cap)
{
    const int k = blockIdx.x * CCL_TILE + threadIdx.x;
    if (k < n_maps) ccl_box_reset(rects + (size_t)k * cap * 4);
}

__global__ __launch_bounds__(CCL_TILE) void k_ccl_init(const double* __restrict__ cur, size_t map_stride, int ncell, int ntile,
                                                       int cols, int thres, int flag, int* __restrict__ par,
                                                       unsigned char* __restrict__ gray, int* __restrict__ rects, int cap)
{
    __shared__ int s_on[CCL_TILE];
    __shared__ int s_wave[CCL_TILE / 64];
    const int k = blockIdx.x / ntile, t = blockIdx.x - k * ntile, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = t * CCL_TILE + tid;
    bool on = false;
    if (i < ncell) {
        const int gi = gate_gray(cur[(size_t)k * map_stride + i]);
        if (gray) gray[(size_t)k * ncell + i] = (unsigned char)gi;
        on = gi >= thres;
    }
    const int x = i % cols, y = i / cols;
    if (flag == 2) {   // the union box of all components is the box of all ON cells
        const unsigned long long any = __ballot(on);
        if (any) ccl_box_fold<true>(on, __ffsll((long long)any) - 1, x, y, rects + (size_t)k * cap * 4);
        return;
    }
    s_on[tid] = on;
    __syncthreads();
    // head of the cell's run of ON cells within this row and tile: an inclusive max-scan of the run starts
    int h = (on && (tid == 0 || x == 0 || !s_on[tid - 1])) ? i : -1;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(h, o);
        if (lane >= o) h = max(h, v);
    }
    if (lane == 63) s_wave[wave] = h;
    __syncthreads();
    for (int w = 0; w < wave; w++) h = max(h, s_wave[w]);
    if (i < ncell) par[(size_t)k * ncell + i] = on ? h : -1;
}

__global__ __launch_bounds__(CCL_TILE) void k_ccl_merge(int* __restrict__ par, int ncell, int ntile, int cols, int conn8)
{
    const int k = blockIdx.x / ntile, t = blockIdx.x - k * ntile;
    const int i = t * CCL_TILE + threadIdx.x;
    if (i >= ncell) return;
    int* p = par + (size_t)k * ncell;
    if (ccl_load(p + i) < 0) return;
    const int x = i % cols, y = i / cols;
    // the cells of a run inside a tile already share their head (k_ccl_init): only a run that crosses a tile edge joins left
    const bool L = x > 0 && ccl_load(p + i - 1) >= 0;
    if (L && threadIdx.x == 0) ccl_union(p, i, i - 1);
    if (y == 0) return;
    // the row above: each ON cell joins the upper neighbours its left neighbour does not already reach
    const int u = i - cols;
    const bool U = ccl_load(p + u) >= 0;
    const bool UL = x > 0 && ccl_load(p + u - 1) >= 0, UR = x + 1 < cols && ccl_load(p + u + 1) >= 0;
    if (!conn8) {
        if (U && !(L && UL)) ccl_union(p, i, u);
    } else if (L) {
        if (!U && UR) ccl_union(p, i, u + 1);
    } else if (U) {
        ccl_union(p, i, u);
    } else {
        if (UL) ccl_union(p, i, u - 1);
        if (UR) ccl_union(p, i, u + 1);
    }
}

__global__ __launch_bounds__(CCL_TILE) void k_ccl_flatten(int* __restrict__ par, int ncell, int ntile, int* __restrict__ tile_roots)
{
    __shared__ int s_cnt[CCL_TILE / 64];
    const int k = blockIdx.x / ntile, t = blockIdx.x - k * ntile, tid = threadIdx.x;
    const int i = t * CCL_TILE + tid;
    int* p = par + (size_t)k * ncell;
    bool root = false;
    if (i < ncell) {
        const int v = ccl_load(p + i);
        if (v >= 0) {
            const int r = ccl_find(p, i);
            if (r != v) ccl_min(p + i, r);
            root = r == i;
        }
    }
    const unsigned long long b = __ballot(root);
    if ((tid & 63) == 0) s_cnt[tid >> 6] = __popcll(b);
    __syncthreads();
    if (tid == 0) tile_roots[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// One workgroup per map: the tiles' root counts become exclusive offsets; the total is the true component count.
__global__ __launch_bounds__(CCL_TILE) void k_ccl_scan(int* __restrict__ tile_roots, int ntile, int* __restrict__ counts,
                                                       int* __restrict__ rects, int cap)
{
    __shared__ int s_wave[CCL_TILE / 64];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* s = tile_roots + (size_t)k * ntile;
    int carry = 0;
    for (int base = 0; base < ntile; base += CCL_TILE) {
        const int j = base + tid;
        const int v = j < ntile ? s[j] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int w = __shfl_up(inc, o);
            if (lane >= o) inc += w;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        int before = carry, total = carry;
        for (int w = 0; w < CCL_TILE / 64; w++) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        if (j < ntile) s[j] = before + inc - v;
        carry = total;
        __syncthreads();
    }
    if (tid == 0) counts[k] = carry;
    int* out = rects + (size_t)k * cap * 4;
    for (int l = tid; l < min(carry, cap); l += CCL_TILE) ccl_box_reset(out + 4 * l);
}

__global__ __launch_bounds__(CCL_TILE) void k_ccl_label(int* __restrict__ par, int ncell, int ntile, const int* __restrict__ tile_roots)
{
    __shared__ int s_cnt[CCL_TILE / 64];
    const int k = blockIdx.x / ntile, t = blockIdx.x - k * ntile, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = t * CCL_TILE + tid;
    int* p = par + (size_t)k * ncell;
    const bool root = i < ncell && p[i] == i;   // only a root's own thread rewrites its slot
    const unsigned long long b = __ballot(root);
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int rank = tile_roots[blockIdx.x] + __popcll(b & ((1ull << lane) - 1));
    for (int w = 0; w < wave; w++) rank += s_cnt[w];
    if (root) p[i] = -2 - rank;
}

__global__ __launch_bounds__(CCL_TILE) void k_ccl_stats(const int* __restrict__ par, int ncell, int ntile, int cols,
                                                        int* __restrict__ rects, int cap)
{
    const int k = blockIdx.x / ntile, t = blockIdx.x - k * ntile;
    const int i = t * CCL_TILE + threadIdx.x;
    const int* p = par + (size_t)k * ncell;
    int lab = -1;
    if (i < ncell) {
        const int v = p[i];   // -1 OFF, <= -2 a root's label, else the root
        if (v != -1) lab = v < -1 ? -2 - v : -2 - p[v];
        if (lab >= cap) lab = -1;
    }
    const int x = i % cols, y = i / cols;
    int* out = rects + (size_t)k * cap * 4;
    unsigned long long todo = __ballot(lab >= 0);
    for (int guard = 0; guard < 64 && todo; guard++) {   // one pass per distinct label in the wave
        const int leader = __ffsll((long long)todo) - 1;
        const int lead_lab = __shfl(lab, leader);
        const bool mine = lab == lead_lab;
        ccl_box_fold<false>(mine, leader, x, y, out + 4 * lead_lab);
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(CCL_TILE) void k_ccl_emit(int* __restrict__ counts, int* __restrict__ rects, int cap, int flag,
                                                       int fw, int fh, int ms, int el, int er, int eu, int ed)
{
    const int k = blockIdx.x, tid = threadIdx.x;
    int* out = rects + (size_t)k * cap * 4;
    int n;
    if (flag == 2) {
        n = out[2] >= 0 ? 1 : 0;
        if (tid == 0) counts[k] = n;
    } else {
        n = min(counts[k], cap);
    }
    for (int l = tid; l < n; l += CCL_TILE) {
        int* r = out + 4 * l;
        const int bx0 = r[0], by0 = r[1], bx1 = r[2], by1 = r[3];
        r[0] = max(bx0 * ms - el, 0);
        r[1] = max(by0 * ms - eu, 0);
        r[2] = min((bx1 + 1) * ms + er, fw);
        r[3] = min((by1 + 1) * ms + ed, fh);
    }
}

// ---- gate statistics of a variability study (nsof_gate_stats_dev) ----------------------------------------------------
// cur [T][F][ncell] are the stacks of T trials, nom [F][ncell] the nominal array's; gated <=> gate_gray(I) >= thres.  One
// launch, two kinds of workgroup (the kind is uniform per workgroup), no atomics -- integer sums, so the result does not
// depend on the order:
//   workgroups [0, n_cnt)    64 consecutive (frame, cell) positions each; wave v counts the trials v, v + 4, ... of its
//                            lane's position (coalesced over the positions), the four partial counts meet in LDS
//   workgroups [n_cnt, ...)  four (trial, frame) pairs each, one per wave: the lanes stride over the cells, a ballot per
//                            round counts the cells whose gated bit differs from the nominal's
constexpr int GS_BLOCK = 256;
__global__ __launch_bounds__(GS_BLOCK) void k_gate_stats(const double* __restrict__ cur, const double* __restrict__ nom, int n_trials,
                                                         size_t n_pos /* F * ncell */, int ncell, size_t n_pairs /* T * F */,
                                                         unsigned n_cnt, int thres, int* __restrict__ counts, int* __restrict__ flips)
{
    __shared__ int s_part[GS_BLOCK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x < n_cnt) {
        const size_t pos = (size_t)blockIdx.x * 64 + lane;
        int c = 0;
        if (pos < n_pos)
            for (int t = wave; t < n_trials; t += GS_BLOCK / 64) c += gate_gray(cur[(size_t)t * n_pos + pos]) >= thres;
        s_part[tid] = c;
        __syncthreads();
        if (wave == 0 && pos < n_pos) counts[pos] = s_part[lane] + s_part[64 + lane] + s_part[128 + lane] + s_part[192 + lane];
        return;
    }
    const size_t pair = (size_t)(blockIdx.x - n_cnt) * (GS_BLOCK / 64) + wave;   // t * F + f
    if (pair >= n_pairs) return;                                                   // (wave-uniform)
    const size_t F = n_pos / (size_t)ncell, f = pair % F;
    const double* a = cur + pair * (size_t)ncell;
    const double* b = nom + f * (size_t)ncell;
    int n = 0;
    for (int c0 = 0; c0 < ncell; c0 += 64) {
        const int c = c0 + lane;
        const bool differs = c < ncell && (gate_gray(a[c]) >= thres) != (gate_gray(b[c]) >= thres);
        n += __popcll(__ballot(differs));
    }
    if (lane == 0) flips[pair] = n;
}

}  // namespace

extern "C" int nsof_gate_stats_dev(nsof_ctx* ctx, const double* d_current, const double* d_nominal, int n_trials, int n_frames,
                                   int rows, int cols, int thres, int* d_counts, int* d_flips)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_current || !d_nominal || !d_counts || !d_flips || n_trials < 1 || n_frames < 1 || rows < 1 || cols < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "bad gate-statistics arguments");
    if ((long long)rows * cols > (1ll << 27))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "gating map %d x %d exceeds 2^27 cells", rows, cols);
    const int ncell = rows * cols;
    const size_t n_pos = (size_t)n_frames * ncell, n_pairs = (size_t)n_trials * n_frames;
    const size_t n_cnt = (n_pos + 63) / 64, n_flip = (n_pairs + GS_BLOCK / 64 - 1) / (GS_BLOCK / 64);
    if (n_cnt + n_flip > 0x7fffffffull)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%d trials of %d maps of %d cells: too large for one launch", n_trials,
                              n_frames, ncell);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_gate_stats, dim3((unsigned)(n_cnt + n_flip)), dim3(GS_BLOCK), 0, ctx->stream, d_current, d_nominal, n_trials,
                       n_pos, ncell, n_pairs, (unsigned)n_cnt, thres, d_counts, d_flips);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// Device twin of nsof_roi_from_surface for n_maps maps at once; everything stays on the context's stream, nothing is
// synchronised.  d_gray (optional): the 8-bit gating maps, [n_maps][rows][cols].
extern "C" int nsof_roi_from_surface_dev(nsof_ctx* ctx, const double* d_current, int n_maps, size_t map_stride, int rows, int cols,
                                         int frame_w, int frame_h, int memsize, int thres, int extend_left, int extend_right,
                                         int extend_upper, int extend_lower, int connectivity, int flag, int max_rects,
                                         int* d_counts, int* d_rects, unsigned char* d_gray)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_current || !d_counts || !d_rects || n_maps < 1 || rows < 1 || cols < 1 || frame_w < 1 || frame_h < 1 || memsize < 1 ||
        (connectivity != 4 && connectivity != 8) || (flag != 1 && flag != 2) || max_rects < 1 || map_stride < (size_t)rows * cols)
        return nsof_set_error(ctx, NSOF_EINVAL, "bad gating arguments");
    if (rows > frame_h / memsize || cols > frame_w / memsize)   // the reference's loop would write outside its transition picture
        return nsof_set_error(ctx, NSOF_ESHAPE, "gating map %d x %d larger than the frame's %d x %d blocks", rows, cols,
                              frame_h / memsize, frame_w / memsize);
    if ((long long)rows * cols > (1ll << 27))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "gating map %d x %d exceeds 2^27 cells", rows, cols);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const int conn8 = connectivity == 8 ? 1 : 0;
    if (rows <= 64 && cols <= 64) {   // one wavefront per map
        hipLaunchKernelGGL(k_roi_gate, dim3(n_maps), dim3(64), 0, ctx->stream, d_current, map_stride, rows, cols, frame_w, frame_h,
                           memsize, thres, extend_left, extend_right, extend_upper, extend_lower, conn8, flag, max_rects,
                           d_counts, d_rects, d_gray);
        NSOF_HIP(ctx, hipGetLastError());
        return NSOF_OK;
    }
    // Larger maps: union-find over the context's workspace (FLAG 1; FLAG 2 needs no scratch), a chunk of maps at a time.
    // A chunk takes what the workspace already holds, at least 64 MiB, at least one map; launches stay below 2^31 threads.
    const int ncell = rows * cols, ntile = (ncell + CCL_TILE - 1) / CCL_TILE;
    const size_t per_map = flag == 1 ? sizeof(int) * ((size_t)ncell + ntile) : 0;
    size_t chunk = std::max<size_t>(1, ((size_t)1 << 23) / ntile);
    int* par = nullptr;
    int* tile_roots = nullptr;
    if (per_map) {
        const size_t budget = std::max(ctx->ws.cap, (size_t)64 << 20);
        chunk = std::min(chunk, std::max<size_t>(1, budget / per_map));
        chunk = std::min(chunk, (size_t)n_maps);
        if (int rc = ctx->ws.reserve(ctx, chunk * per_map)) return rc;
        par = (int*)ctx->ws.p;
        tile_roots = par + chunk * ncell;
    }
    for (int m0 = 0; m0 < n_maps; m0 += (int)chunk) {
        const int c = (int)std::min<size_t>(chunk, (size_t)(n_maps - m0));
        const double* cur = d_current + (size_t)m0 * map_stride;
        int* counts = d_counts + m0;
        int* rects = d_rects + (size_t)m0 * max_rects * 4;
        unsigned char* gray = d_gray ? d_gray + (size_t)m0 * ncell : nullptr;
        const dim3 cells((unsigned)c * ntile), tile(CCL_TILE);
        if (flag == 2)
            hipLaunchKernelGGL(k_ccl_box_reset, dim3((c + CCL_TILE - 1) / CCL_TILE), tile, 0, ctx->stream, c, rects, max_rects);
        hipLaunchKernelGGL(k_ccl_init, cells, tile, 0, ctx->stream, cur, map_stride, ncell, ntile, cols, thres, flag, par, gray,
                           rects, max_rects);
        if (flag == 1) {
            hipLaunchKernelGGL(k_ccl_merge, cells, tile, 0, ctx->stream, par, ncell, ntile, cols, conn8);
            hipLaunchKernelGGL(k_ccl_flatten, cells, tile, 0, ctx->stream, par, ncell, ntile, tile_roots);
            hipLaunchKernelGGL(k_ccl_scan, dim3(c), tile, 0, ctx->stream, tile_roots, ntile, counts, rects, max_rects);
            hipLaunchKernelGGL(k_ccl_label, cells, tile, 0, ctx->stream, par, ncell, ntile, tile_roots);
            hipLaunchKernelGGL(k_ccl_stats, cells, tile, 0, ctx->stream, par, ncell, ntile, cols, rects, max_rects);
        }
        hipLaunchKernelGGL(k_ccl_emit, dim3(c), tile, 0, ctx->stream, counts, rects, max_rects, flag, frame_w, frame_h, memsize,
                           extend_left, extend_right, extend_upper, extend_lower);
        NSOF_HIP(ctx, hipGetLastError());
    }
    return NSOF_OK;
}
