// FarnebackUpdateFlow_GaussianBlur (OPTFLOW_FARNEBACK_GAUSSIAN): the second kernel of the unfused iteration with a
// separable Gaussian window in place of the box.  One launch does the vertical pass, the horizontal pass and the 2x2 solve.
//
// Arithmetic (upstream's, restated in tests/farneback_gauss.py), m = winsize / 2, taps k[0..m] formed on the host:
//   v    = M[y][x] * k[0];  for i = 1..m:  v += (M[min(y+i,H-1)][x] + M[max(y-i,0)][x]) * k[i]      per plane of M, float
//   h    = v[x] * k[0];     for i = 1..m:  h += k[i] * (v[max(x-i,0)] + v[min(x+i,W-1)])            float
//   idet = 1. / ((double)(g11*g22 - g12*g12) + 1e-3),  flow = ((float)((double)(g11*h2 - g12*h1) * idet), (g22*h1 - g12*h2) ..)
// Every product and sum is rounded on its own (-ffp-contract=off); the reciprocal is the correctly rounded double one.
// M: planar [pair][5][H][W] as k_update_matrices writes it; flow: interleaved [pair][H][W][2], written in place (the kernel
// reads M only).  The lagged stripe update of M upstream interleaves with the row loop is the next iteration's
// k_update_matrices: it touches only rows no later window reads.
//
// LDS form (m <= NSOF_GAUSS_LDS_MAX_M): a workgroup of 256 threads owns a tile of GS_TY x GS_TX outputs.  One plane at a
// time, the tile and its halo of m rows and columns ((GS_TY+2m)(GS_TX+2m) floats, edges replicated by clamped loads) go to
// LDS, through registers that are loaded one plane ahead; the vertical pass writes GS_TY rows of v (halo columns included) to a second LDS array; the horizontal pass keeps
// its results in registers (2 x 4 outputs x 5 planes per thread).  Both passes give a thread 4 neighbouring outputs along
// the pass direction and slide two 4-wide register windows outwards from the centre, so step i costs 2 LDS reads for 4
// outputs while every output still adds its pairs in the order i = 1..m.  v is stored with the column's low two bits as
// the slow index ([row][x & 3][x >> 2]): the horizontal pass, whose lanes are 4 columns apart, then reads consecutive
// words; GS_VS % 32 == 24 and GS_VROW % 32 == 16 keep the writes of 32 neighbouring columns and the reads of two
// neighbouring rows on distinct banks.
// General form (larger m, up to NSOF_GAUSS_MAX_M): one thread per pixel with clamped loads straight from memory,
// (2m+1)^2 of them per plane.  It is there for completeness and is slow.
#include <cmath>

#include "nsof_internal.h"

namespace {

constexpr int GS_TX = 64, GS_TY = 32;
constexpr int GS_VS = (GS_TX + 2 * NSOF_GAUSS_LDS_MAX_M) / 4;   // words per (x & 3) plane of a row of v
constexpr int GS_VROW = 4 * GS_VS + 16;
static_assert(GS_VS % 32 == 24 && GS_VROW % 32 == 16, "bank layout of v (see above)");
constexpr int GS_LOADS = (GS_TY + 2 * NSOF_GAUSS_LDS_MAX_M) / 4;   // tile rows (with halo) per wave, at most
static_assert(GS_TX == 64 && GS_TY == 32, "the thread mapping below: 16 column groups x 16 rows, two rows per thread");

__device__ __forceinline__ float2 gauss_solve(float g11, float g12, float g22, float h1, float h2)
{
    const double idet = 1. / ((double)(g11 * g22 - g12 * g12) + 1e-3);
    return make_float2((float)((double)(g11 * h2 - g12 * h1) * idet), (float)((double)(g22 * h1 - g12 * h2) * idet));
}

__global__ __launch_bounds__(256) void k_gauss_blur_solve(const float* __restrict__ M, int W, int H, int m, nsof_gauss_taps taps,
                                                           float* __restrict__ flow)
{
    extern __shared__ float gs_lds[];
    const int CW = GS_TX + 2 * m, RH = GS_TY + 2 * m;
    float* raw = gs_lds;            // [RH][CW]: the plane's tile with its halo
    float* vb = gs_lds + RH * CW;   // [GS_TY][GS_VROW]: the vertical pass of the tile's rows, halo columns included
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int x0 = blockIdx.x * GS_TX, y0 = blockIdx.y * GS_TY;
    const size_t plane = (size_t)W * H;
    const float* Mz = M + (size_t)blockIdx.z * 5 * plane;
    const int cg = tid & 15, r0 = tid >> 4;   // horizontal pass: columns 4 cg .. 4 cg + 3 of rows r0 and r0 + 16
    const float k0 = taps.k[0];

    // The tile's loads: wave w takes rows w, w + 4, ... and a lane columns lane and lane + 64.  All of a plane's loads are
    // issued together into registers, and those of plane c + 1 before the passes of plane c, so their latency is covered
    // by the arithmetic (loaded and stored one at a time, the kernel took 3.8 instead of 2.4 ms on 64 1080p pairs, window 15).  Row and
    // column are clamped, so a load beyond the tile's halo reads valid memory and is just not stored.
    float pre[GS_LOADS][2];
    auto fetch = [&](int c) {
        const float* Mc = Mz + c * plane;
#pragma unroll
        for (int u = 0; u < GS_LOADS; u++) {
            const int r = wave + 4 * u;
            if (r < RH) {
                const float* row = Mc + (size_t)clampi(y0 - m + r, 0, H - 1) * W;
                pre[u][0] = row[clampi(x0 - m + lane, 0, W - 1)];
                pre[u][1] = row[clampi(x0 - m + lane + 64, 0, W - 1)];
            }
        }
    };
    fetch(0);

    float res[2][4][5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
#pragma unroll
        for (int u = 0; u < GS_LOADS; u++) {
            const int r = wave + 4 * u;
            if (r < RH) {
                raw[r * CW + lane] = pre[u][0];
                if (lane + 64 < CW) raw[r * CW + lane + 64] = pre[u][1];
            }
        }
        if (c < 4) fetch(c + 1);
        __syncthreads();
        // vertical pass: a thread takes tile rows 4 rg .. 4 rg + 3 of one column
        for (int rg = wave; rg < GS_TY / 4; rg += 4)
            for (int cc = lane; cc < CW; cc += 64) {
                const float* col = raw + (4 * rg + m) * CW + cc;   // the first of the 4 centres
                float v[4], up[4], dn[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    up[q] = dn[q] = col[q * CW];
                    v[q] = up[q] * k0;
                }
#pragma unroll 2
                for (int i = 1; i <= m; i++) {
                    up[0] = up[1]; up[1] = up[2]; up[2] = up[3]; up[3] = col[(3 + i) * CW];
                    dn[3] = dn[2]; dn[2] = dn[1]; dn[1] = dn[0]; dn[0] = col[-i * CW];
                    const float k = taps.k[i];
#pragma unroll
                    for (int q = 0; q < 4; q++) v[q] += (up[q] + dn[q]) * k;
                }
#pragma unroll
                for (int q = 0; q < 4; q++) vb[(4 * rg + q) * GS_VROW + (cc & 3) * GS_VS + (cc >> 2)] = v[q];
            }
        __syncthreads();
        // horizontal pass: v column of output column x is x + m; column 4 cg + t lies at [(t & 3)][cg + (t >> 2)]
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const float* vr = vb + (r0 + 16 * j) * GS_VROW + cg;
            float h[4], rt[4], lf[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int t = m + p;
                rt[p] = lf[p] = vr[(t & 3) * GS_VS + (t >> 2)];
                h[p] = rt[p] * k0;
            }
#pragma unroll 2
            for (int i = 1; i <= m; i++) {
                const int tr = m + 3 + i, tl = m - i;
                rt[0] = rt[1]; rt[1] = rt[2]; rt[2] = rt[3]; rt[3] = vr[(tr & 3) * GS_VS + (tr >> 2)];
                lf[3] = lf[2]; lf[2] = lf[1]; lf[1] = lf[0]; lf[0] = vr[(tl & 3) * GS_VS + (tl >> 2)];
                const float k = taps.k[i];
#pragma unroll
                for (int p = 0; p < 4; p++) h[p] += k * (lf[p] + rt[p]);
            }
#pragma unroll
            for (int p = 0; p < 4; p++) res[j][p][c] = h[p];
        }
        // the next plane's stores overwrite raw only (every thread is past the vertical pass); its vertical pass writes vb
        // after the barrier that follows those stores, which a thread reaches after its reads of vb above
    }

    float2* fz = reinterpret_cast<float2*>(flow) + (size_t)blockIdx.z * plane;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int y = y0 + r0 + 16 * j, x = x0 + 4 * cg;
        if (y >= H) continue;
        float2* dst = fz + (size_t)y * W + x;
#pragma unroll
        for (int p = 0; p < 4; p++)
            if (x + p < W) dst[p] = gauss_solve(res[j][p][0], res[j][p][1], res[j][p][2], res[j][p][3], res[j][p][4]);
    }
}

__global__ __launch_bounds__(256) void k_gauss_blur_solve_general(const float* __restrict__ M, int W, int H, int m,
                                                                   nsof_gauss_taps taps, float* __restrict__ flow)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t plane = (size_t)W * H;
    const float* Mz = M + (size_t)blockIdx.z * 5 * plane;
    auto vertical = [&](const float* Mc, int xc) {
        float v = Mc[(size_t)y * W + xc] * taps.k[0];
        for (int i = 1; i <= m; i++)
            v += (Mc[(size_t)min(y + i, H - 1) * W + xc] + Mc[(size_t)max(y - i, 0) * W + xc]) * taps.k[i];
        return v;
    };
    float g[5];
    for (int c = 0; c < 5; c++) {
        const float* Mc = Mz + c * plane;
        float h = vertical(Mc, x) * taps.k[0];
        for (int i = 1; i <= m; i++) h += taps.k[i] * (vertical(Mc, max(x - i, 0)) + vertical(Mc, min(x + i, W - 1)));
        g[c] = h;
    }
    reinterpret_cast<float2*>(flow)[(size_t)blockIdx.z * plane + (size_t)y * W + x] = gauss_solve(g[0], g[1], g[2], g[3], g[4]);
}

}  // namespace

// Upstream's taps: t_i = (float)exp(-i*i / (2 sigma^2)) with sigma = 0.3 m, normalised by the double sum 1 + sum 2 t_i.
static void gauss_host_taps(int m, nsof_gauss_taps* t)
{
    const double sigma = m * 0.3;
    double s = 1;
    t->k[0] = 1.f;
    for (int i = 1; i <= m; i++) {
        const float ti = (float)std::exp(-i * i / (2 * sigma * sigma));
        t->k[i] = ti;
        s += ti * 2;
    }
    s = 1. / s;
    for (int i = 0; i <= m; i++) t->k[i] = (float)(t->k[i] * s);
    for (int i = m + 1; i <= NSOF_GAUSS_MAX_M; i++) t->k[i] = 0.f;
}

int nsof_launch_gauss_blur_solve(nsof_ctx* ctx, int n_pairs, const float* M, int W, int H, int winsize, float* flow)
{
    const int m = winsize / 2;
    if (m < 1 || m > NSOF_GAUSS_MAX_M)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "winsize=%d outside 2..%d for the Gaussian window", winsize, 2 * NSOF_GAUSS_MAX_M + 1);
    const int rows = m <= NSOF_GAUSS_LDS_MAX_M ? GS_TY : 4;   // image rows per workgroup, on gridDim.y
    if ((H + rows - 1) / rows > 65535) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "height %d too large for the Gaussian window", H);
    nsof_gauss_taps taps;
    gauss_host_taps(m, &taps);
    nsof_prof_scope ps(ctx, NSOF_K_BLUR);
    if (m <= NSOF_GAUSS_LDS_MAX_M) {
        const size_t lds = ((size_t)(GS_TY + 2 * m) * (GS_TX + 2 * m) + (size_t)GS_TY * GS_VROW) * sizeof(float);
        hipLaunchKernelGGL(k_gauss_blur_solve, dim3((W + GS_TX - 1) / GS_TX, (H + GS_TY - 1) / GS_TY, n_pairs), dim3(256), lds,
                           ctx->stream, M, W, H, m, taps, flow);
    } else {
        hipLaunchKernelGGL(k_gauss_blur_solve_general, dim3((W + 63) / 64, (H + 3) / 4, n_pairs), dim3(256), 0, ctx->stream, M, W,
                           H, m, taps, flow);
    }
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
