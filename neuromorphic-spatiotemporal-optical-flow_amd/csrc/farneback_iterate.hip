// Farneback inner iteration, fused: matrix update (warped R1) + box blur + 2x2 solve in ONE kernel (k_iterate_q, the
// per-pixel window sums of the fast row-sum mode; the library's running row-sum order is k_iterate_x).
//
// Reference arithmetic: FarnebackUpdateMatrices followed by FarnebackUpdateFlow_Blur of the library behind
// cv2.calcOpticalFlowFarneback (/root/reference/optical_flow_seg.py:203).  The unfused pair of kernels
// (k_update_matrices + k_blur_solve) moves 68 + 28 = 96 B/px per iteration through HBM because the
// 5-plane matrix M is written and read back.  Here M never leaves the CU: a workgroup owns a strip of 256 image
// columns (SW outputs + m halo columns per side) and walks down the image, FOUR rows per step -- the column sums are
// running sums from row 0 (each row adds double(float(M[y+m] - M[y-m-1])): the float rounding of that difference is
// part of the reference arithmetic), so rows must be visited in order.
//   waves 0-3   consumers: column sums of 4 rows (thread <-> column), then row sums + solve, thread <-> 4 adjacent
//               pixels of one row (first pixel summed directly, the next three sliding)
//   waves 4-7 / 8-11  producers A / B: rows 0,1 / 2,3 of every step (bilinear gather of R1 at x+flow), the loads of
//               their next two steps in flight
// Four rows rather than two: a step's work per wave is one dependent chain -- LDS round trips, the double-precision
// solve, a gather's address arithmetic -- that lasts about as long whatever it carries, so more independent work per
// chain is what fills VALU, LDS and the vector L1 (the 2-row form: docs/HISTORY_r1_r3.md).
// The column sums are single-buffered (4 rows x 5 planes x 256 doubles = 40 KB) so that the ring of 2m+9 rows of M
// (23 x 5 KB at winsize 15) still fits the 160 KB of LDS: two barriers per step (column sums visible / consumed).
// Producers write the first row of step t+1 while the consumers form the column sums of step t, and its second row
// while they solve; the slots those rows overwrite left the window long before.  Pixels 4k+2, 4k+3 of a row reach
// their row sums by sliding instead of by a direct sum: same double-precision values up to their last bit.
//
// HBM traffic per pixel per iteration: R0 20 + R1 ~20 + flow 8 read, flow 8 written = 56 B (+ halo).
#include "iterate_common.h"

namespace {

template <int MH>
struct QGeom {
    static constexpr int COLS = 256, RB = 4;
    static constexpr int RL = 2 * MH + 1 + 2 * RB;
    static constexpr int SW = (COLS - 2 * MH) & ~3;         // a solve thread owns 4 whole pixels
    // Column sums of one (row, plane): the solve threads read 4 adjacent columns each, i.e. lanes 4 doubles apart -- a
    // 4-way bank conflict on a plain row (PMC: 32 % of the kernel's LDS cycles).  Stored as four sub-rows by
    // (column mod 4), 68 doubles apart: a lane's reads (consecutive lanes, consecutive doubles) and the column-sum
    // writes (ds_write_b64: 16 lanes per LDS cycle over 32 banks; 136 dwords = 8 mod 32) are both conflict free.
    static constexpr int SVSUB = COLS / 4 + 4, SVW = 3 * SVSUB + COLS / 4;
    static constexpr size_t SV_BYTES = sizeof(double) * RB * 5 * SVW;
    static constexpr size_t SMEM = SV_BYTES + sizeof(float) * RL * 5 * COLS;
    __host__ __device__ static constexpr int svi(int col) { return (col & 3) * SVSUB + (col >> 2); }
};

template <int MH, int GP, int TS, int RR>
__device__ __forceinline__ void q_produce(RowIn (&in)[2][2], float2 (&dd)[2][2], float2 (&fl)[2][2], float (*mring)[5][QGeom<MH>::COLS],
                                          const Planes& R0, const Planes& R1, const FlowSrc& F, int W, int H, int xc,
                                          int col, int t, int yb)
{
    constexpr int RL = QGeom<MH>::RL;
    const int i = 4 * t + MH + 2 * GP + RR;                  // stream index of this row (row yb + i of the image)
    float Mn[5];
    matrix_from(in[TS][RR], dd[TS][RR].x, dd[TS][RR].y, xc, min(yb + i, H - 1), W, H, Mn);
    const int slot = (i + MH + 1) % RL;
#pragma unroll
    for (int c = 0; c < 5; c++) mring[slot][c][col] = Mn[c];
    issue_row(in[TS][RR], R0, R1, W, H, xc, min(yb + i + 8, H - 1), fl[TS][RR]);              // the same row of step t+2
    dd[TS][RR] = fl[TS][RR];
    fl[TS][RR] = F.fetch(min(yb + i + 16, H - 1));                                            // its flow for step t+4
}

template <int MH, int GP>
__device__ __forceinline__ void q_producer_loop(float (*mring)[5][QGeom<MH>::COLS], const Planes& R0, const Planes& R1,
                                                const FlowSrc& F, int W, int H, int xc, int col, int nsteps, int yb)
{
    RowIn in[2][2];
    float2 dd[2][2], fl[2][2];   // the flow of the rows in `in`, and of the rows issued next
#pragma unroll
    for (int ts = 0; ts < 2; ts++)
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            const int r = min(yb + 4 * ts + MH + 2 * GP + rr, H - 1);
            dd[ts][rr] = F.fetch(r);
            issue_row(in[ts][rr], R0, R1, W, H, xc, r, dd[ts][rr]);
        }
#pragma unroll
    for (int ts = 0; ts < 2; ts++)
#pragma unroll
        for (int rr = 0; rr < 2; rr++) fl[ts][rr] = F.fetch(min(yb + 4 * (ts + 2) + MH + 2 * GP + rr, H - 1));
    // Barriers (all roles alike): B_init, then B1(t), B2(t) for every step t.
    //   before B_init          both rows of step 0
    //   B_init .. B1(0)        first row of step 1            (consumers: column sums of step 0)
    //   B1(t) .. B2(t)         second row of step t+1         (consumers: row sums + solve of step t)
    //   B2(t) .. B1(t+1)       first row of step t+2          (consumers: column sums of step t+1)
    q_produce<MH, GP, 0, 0>(in, dd, fl, mring, R0, R1, F, W, H, xc, col, 0, yb);
    q_produce<MH, GP, 0, 1>(in, dd, fl, mring, R0, R1, F, W, H, xc, col, 0, yb);
    __syncthreads();
    q_produce<MH, GP, 1, 0>(in, dd, fl, mring, R0, R1, F, W, H, xc, col, 1, yb);
    for (int tb = 0; tb < nsteps; tb += 2) {
        __syncthreads();                                                             // B1(tb)
        q_produce<MH, GP, 1, 1>(in, dd, fl, mring, R0, R1, F, W, H, xc, col, tb + 1, yb);
        __syncthreads();                                                             // B2(tb)
        q_produce<MH, GP, 0, 0>(in, dd, fl, mring, R0, R1, F, W, H, xc, col, tb + 2, yb);
        if (tb + 1 >= nsteps) break;
        __syncthreads();                                                             // B1(tb+1)
        q_produce<MH, GP, 0, 1>(in, dd, fl, mring, R0, R1, F, W, H, xc, col, tb + 2, yb);
        __syncthreads();                                                             // B2(tb+1)
        q_produce<MH, GP, 1, 0>(in, dd, fl, mring, R0, R1, F, W, H, xc, col, tb + 3, yb);
    }
}

template <int MH>
__device__ __forceinline__ void q_consumer_loop(float (*mring)[5][QGeom<MH>::COLS], void* sv_raw, const Planes& R0,
                                                const Planes& R1, const FlowSrc& F, float2* Fout, size_t fpitch, int W,
                                                int H, int x0, int xc, int col, int nsteps, double scale, int yb, int ye)
{
    using G = QGeom<MH>;
    constexpr int RL = G::RL, SW = G::SW, TPR = G::COLS / 4;   // TPR solve threads per row
    double (*sv)[5][G::SVW] = reinterpret_cast<double (*)[5][G::SVW]>(sv_raw);   // [4 rows][5 planes]
    double vs[5];
    if (yb > 0) {
        // a row band that starts inside the image (opt-in NSOF_OPT_ROW_BANDS): the window of row yb-1, rows
        // yb-m-1 .. yb+m-1, is summed directly -- the library's column sums are ONE running sum from row 0, so this
        // start differs from it in the sums' last bits (same class as the row-sum order).
        RowIn t[2];
        float2 d[2];
        const int r0 = max(yb - MH - 1, 0);
        d[0] = F.fetch(r0);
        issue_row(t[0], R0, R1, W, H, xc, r0, d[0]);
#pragma unroll
        for (int c = 0; c < 5; c++) vs[c] = 0.;
#pragma unroll
        for (int j = 0; j <= 2 * MH; j++) {
            const int r = clampi(yb - MH - 1 + j, 0, H - 1);
            if (j < 2 * MH) {
                const int rn = clampi(yb - MH + j, 0, H - 1);
                d[(j + 1) & 1] = F.fetch(rn);
                issue_row(t[(j + 1) & 1], R0, R1, W, H, xc, rn, d[(j + 1) & 1]);
            }
            float Mi[5];
            matrix_from(t[j & 1], d[j & 1].x, d[j & 1].y, xc, r, W, H, Mi);
#pragma unroll
            for (int c = 0; c < 5; c++) {
                vs[c] += (double)Mi[c];
                mring[j][c][col] = Mi[c];
            }
        }
    } else {
        // prologue: rows 0..m-1 enter the sums; the m+1 rows above the image replicate row 0.
        // ring slot of stream index i is (i + m + 1) % RL.
        RowIn t;
        float M0[5];
        float2 d = F.fetch(0);
        issue_row(t, R0, R1, W, H, xc, 0, d);
        matrix_from(t, d.x, d.y, xc, 0, W, H, M0);
#pragma unroll
        for (int c = 0; c < 5; c++) {
            vs[c] = (double)(M0[c] * (float)(MH + 2));   // float product, as "srow0[x]*(m+2)"
#pragma unroll
            for (int j = 0; j <= MH + 1; j++) mring[j][c][col] = M0[c];   // stream indices -m-1 .. 0
        }
#pragma unroll
        for (int i = 1; i < MH; i++) {
            float Mi[5];
            const int r = min(i, H - 1);
            d = F.fetch(r);
            issue_row(t, R0, R1, W, H, xc, r, d);
            matrix_from(t, d.x, d.y, xc, r, W, H, Mi);
#pragma unroll
            for (int c = 0; c < 5; c++) {
                vs[c] += (double)Mi[c];
                mring[i + MH + 1][c][col] = Mi[c];
            }
        }
    }
    __syncthreads();   // B_init: step 0 is in the ring
    const int hrow = col / TPR, t4 = col % TPR;   // solve phase: COLS/4 threads per row, 4 pixels each
    int slot_new = (2 * MH + 1) % RL;           // stream index m    -> slot 2m+1
    int slot_old = 0;                           // stream index -m-1 -> slot 0
    for (int t = 0; t < nsteps; t++) {
        // column sums: four more rows enter the window of this thread's column
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int c = 0; c < 5; c++) {
                const float d = mring[slot_new][c][col] - mring[slot_old][c][col];
                vs[c] += (double)d;
                sv[q][c][G::svi(col)] = vs[c];
            }
            slot_new = slot_new + 1 == RL ? 0 : slot_new + 1;
            slot_old = slot_old + 1 == RL ? 0 : slot_old + 1;
        }
        __syncthreads();   // B1(t): column sums of step t visible
        const int yo = yb + 4 * t + hrow, xo = x0 + 4 * t4;
        if (4 * t4 < SW && yo < ye && xo < W) {
            const double (*svr)[G::SVW] = sv[hrow];
            auto at = [&](int c, int j) { return svr[c][(j & 3) * G::SVSUB + t4 + (j >> 2)]; };   // column 4 t4 + j
            double g[5];
            float2 o[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (p == 0) {
#pragma unroll
                    for (int c = 0; c < 5; c++) {
                        double a = 0;
#pragma unroll
                        for (int j = 0; j <= 2 * MH; j++) a += at(c, j);
                        g[c] = a;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 5; c++) g[c] += at(c, p + 2 * MH) - at(c, p - 1);
                }
                o[p] = nsof_flow_solve(g[0], g[1], g[2], g[3], g[4], scale);
            }
            float2* dst = Fout + (size_t)yo * fpitch + xo;
            if (xo + 3 < W && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                nsof_store_stream4(reinterpret_cast<float*>(dst), o[0].x, o[0].y, o[1].x, o[1].y);
                nsof_store_stream4(reinterpret_cast<float*>(dst + 2), o[2].x, o[2].y, o[3].x, o[3].y);
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (xo + p < W) dst[p] = o[p];
            }
        }
        __syncthreads();   // B2(t): column sums consumed, the buffer may be rewritten
    }
}

// The double* argument is unused: a reserved slot that keeps the argument layout (and band_rows' offset) fixed.
template <int MH, bool HET>
__global__ __launch_bounds__(3 * QGeom<MH>::COLS) void k_iterate_q(const float* __restrict__ R0b,
                                                                   const float* __restrict__ R1b, size_t pair_stride,
                                                                   const float* __restrict__ flow_in,
                                                                   float* __restrict__ flow_out, int W, int H,
                                                                   int block_size, const nsof_het_item* __restrict__ items,
                                                                   int het_final, double* __restrict__ = nullptr,
                                                                   int band_rows = 0)
{
    using G = QGeom<MH>;
    constexpr int SW = G::SW, COLS = G::COLS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_q[];
    void* sv = smem_q;                                                                          // [4 rows][5][SVW] doubles
    float (*mring)[5][COLS] = reinterpret_cast<float (*)[5][COLS]>(smem_q + G::SV_BYTES);       // [RL]
    const int tid = threadIdx.x, col = tid % COLS;
    const int role = __builtin_amdgcn_readfirstlane(tid / COLS);   // wave-uniform: 0 consumers, 1/2 producers A/B
    int strip = blockIdx.x, pair = blockIdx.z;
    size_t fpitch = (size_t)W;
    if constexpr (HET) {
        const nsof_het_item& it = items[blockIdx.z];
        W = it.wk;
        H = it.hk;
        if (blockIdx.x * SW >= W) return;   // block-uniform, before any barrier
        R0b += it.offR;
        R1b = R0b + 5 * (size_t)W * H;
        pair_stride = 0;
        pair = 0;
        flow_in += 2 * it.offF;
        if (het_final) {
            flow_out = it.out;
            fpitch = (size_t)it.out_pitch;
        } else {
            flow_out += 2 * it.offF;
            fpitch = (size_t)W;
        }
    } else {
        // XCD-aware placement: workgroups are dealt round-robin to the 8 XCDs (linear id % 8), each with its own L2.
        // With the natural (strip, pair) order the strips of a pair land on different L2s and their shared halo
        // columns and gather rows are fetched once per XCD; remapped, an XCD owns whole pairs.
        const unsigned total = gridDim.x * gridDim.z;
        if ((total & 7u) == 0 && gridDim.y == 1) {
            const unsigned lin = blockIdx.x + gridDim.x * blockIdx.z;
            const unsigned j = (lin & 7u) * (total >> 3) + (lin >> 3);
            pair = (int)(j / gridDim.x);
            strip = (int)(j - (unsigned)pair * gridDim.x);
        }
    }
    const int x0 = strip * SW;
    const int xc = clampi(x0 - MH + col, 0, W - 1);
    const size_t plane = (size_t)W * H;
    const Planes R0 = planes_of(R0b + (size_t)pair * pair_stride, plane);
    const Planes R1 = planes_of(R1b + (size_t)pair * pair_stride, plane);
    FlowSrc F;
    F.base = reinterpret_cast<const char*>(flow_in) + (size_t)pair * plane * 8;
    F.W = (unsigned)W;
    F.xc = (unsigned)xc;
    float2* Fout = reinterpret_cast<float2*>(flow_out) + (size_t)pair * plane;
    // band_rows > 0 (a multiple of 4): blockIdx.y owns rows [yb, ye) only -- more workgroups for a small batch
    int yb = 0, ye = H;
    if (band_rows > 0) {
        yb = blockIdx.y * band_rows;
        ye = min(H, yb + band_rows);
        if (yb >= H) return;   // block-uniform, before any barrier
    }
    const int nsteps = (ye - yb + 3) / 4;
    if (role == 0)
        q_consumer_loop<MH>(mring, sv, R0, R1, F, Fout, fpitch, W, H, x0, xc, col, nsteps, 1. / (block_size * block_size),
                            yb, ye);
    else if (role == 1)
        q_producer_loop<MH, 0>(mring, R0, R1, F, W, H, xc, col, nsteps, yb);
    else
        q_producer_loop<MH, 1>(mring, R0, R1, F, W, H, xc, col, nsteps, yb);
}

template <int MH>
int launch_iterate_q(nsof_ctx* ctx, int n_pairs, const float* R0, const float* R1, size_t pair_stride,
                     const float* flow_in, float* flow_out, int W, int H, int winsize)
{
    using G = QGeom<MH>;
    if (int rc = lds_opt_in(ctx, k_iterate_q<MH, false>, G::SMEM)) return rc;
    dim3 grid((W + G::SW - 1) / G::SW, 1, n_pairs);
    // Opt-in row bands (NSOF_OPT_ROW_BANDS): a small batch has too few (strip, pair) workgroups for 256 CUs and each
    // walks the whole height; bands of rows add workgroups at the price of 2m+1 extra rows per band.  1 = automatic
    // (bands no shorter than 32 rows, until the launch has about two workgroups per CU), >= 4 = that many rows.
    // Automatic mode only from winsize 9 up: with small windows the 2x2 systems are rank deficient often enough that a
    // band's restart shows in the 4th decimal of many pixels (parity soak, docs/HISTORY_r1_r3.md section 5.1); an explicit row
    // count is taken at its word.
    int band_rows = 0;
    if (ctx->opt_row_bands > 0) {
        if (ctx->opt_row_bands >= 4) {
            band_rows = (ctx->opt_row_bands + 3) & ~3;
        } else if (winsize < 9) {
            band_rows = 0;
        } else {
            const int want = (512 + (int)(grid.x * grid.z) - 1) / (int)(grid.x * grid.z);   // bands per strip
            band_rows = std::max(32, ((H + want - 1) / want + 3) & ~3);
        }
        if (band_rows >= H) band_rows = 0;
    }
    if (band_rows > 0) grid.y = (H + band_rows - 1) / band_rows;
    hipLaunchKernelGGL((k_iterate_q<MH, false>), grid, dim3(768), G::SMEM, ctx->stream, R0, R1, pair_stride, flow_in,
                       flow_out, W, H, winsize, nullptr, 0, nullptr, band_rows);
    return NSOF_OK;
}

template <int MH>
int launch_iterate_q_het(nsof_ctx* ctx, int n_items, const nsof_het_item* items, int max_w, const float* R,
                         const float* flow_in, float* flow_out, bool final, int winsize)
{
    using G = QGeom<MH>;
    if (int rc = lds_opt_in(ctx, k_iterate_q<MH, true>, G::SMEM)) return rc;
    dim3 grid((max_w + G::SW - 1) / G::SW, 1, n_items);
    hipLaunchKernelGGL((k_iterate_q<MH, true>), grid, dim3(768), G::SMEM, ctx->stream, R, R, (size_t)0, flow_in, flow_out,
                       0, 0, winsize, items, final ? 1 : 0);
    return NSOF_OK;
}

}  // namespace

// flow_in and flow_out must be different buffers (rows y+m of flow_in are read while row y of flow_out is written).
int nsof_launch_iterate(nsof_ctx* ctx, int n_pairs, const float* R0, const float* R1, size_t pair_stride,
                        const float* flow_in, float* flow_out, int W, int H, int winsize)
{
    const int m = winsize / 2;
    if (m < 1 || m > 7) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "fused iteration supports winsize 2..15");
    nsof_prof_scope ps(ctx, NSOF_K_ITERATE);
    int rc = NSOF_OK;
    nsof_with_int<1, 7>(m, [&](auto mh) {
        rc = launch_iterate_q<decltype(mh)::value>(ctx, n_pairs, R0, R1, pair_stride, flow_in, flow_out, W, H, winsize);
    });
    if (rc) return rc;
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// Work-list twin of nsof_launch_iterate (winsize 2..15).
int nsof_launch_iterate_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, const float* R,
                            const float* flow_in, float* flow_out, bool final, int winsize)
{
    const int m = winsize / 2;
    if (m < 1 || m > 7) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "work-list iteration supports winsize 2..15");
    nsof_prof_scope ps(ctx, NSOF_K_ITERATE);
    int rc = NSOF_OK;
    nsof_with_int<1, 7>(m, [&](auto mh) {
        rc = launch_iterate_q_het<decltype(mh)::value>(ctx, n_items, d_items, max_w, R, flow_in, flow_out, final, winsize);
    });
    if (rc) return rc;
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
