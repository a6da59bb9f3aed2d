// Farneback dense optical flow, the unfused box-window solve (FarnebackUpdateFlow_Blur) for gfx950 (CDNA4, wave64):
// k_blur_solve and the exact-order pair k_blur_colsum + k_blur_rowsolve, for the windows and calls the fused iterations
// (farneback_iterate*.hip) do not take.  M planar [n][5][h][w] f32, flow [n][h][w][2].
#include "nsof_internal.h"

namespace {

// ---------------------------------------------------------------------------------------
// FarnebackUpdateFlow_Blur: (2m+1)^2 box sums of the 5 planes of M + per-pixel 2x2 solve.
//
// Strip walker over the full image height (the column sums are a running sum from row 0:
// each row adds double(float(M[y+m] - M[y-m-1])) -- the float rounding of the difference is
// part of the reference arithmetic and is reproduced).  thread <-> column keeps the 5
// column sums in registers as doubles; 4 rows per step go to LDS; wave <-> row, lane <-> 4
// pixels forms the row sums (first pixel direct, then sliding) and solves.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_blur_solve(const float* __restrict__ M, int W, int H, int m, int block_size,
                                                     float* __restrict__ flow)
{
    __shared__ double sv[4][5][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int SW = (256 - 2 * m) & ~3;  // multiple of 4: every lane owns 4 whole pixels
    const int x0 = blockIdx.x * SW;
    const size_t plane = (size_t)W * H;
    const float* Mz = M + (size_t)blockIdx.z * 5 * plane;
    float2* fz = reinterpret_cast<float2*>(flow) + (size_t)blockIdx.z * plane;
    const int xc = clampi(x0 - m + tid, 0, W - 1);
    const float* Mc = Mz + xc;
    const double scale = 1. / (block_size * block_size);

    double vs[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        vs[c] = (double)(Mc[c * plane] * (float)(m + 2));  // float product, as "srow0[x]*(m+2)"
        for (int y = 1; y < m; y++) vs[c] += (double)Mc[c * plane + (size_t)min(y, H - 1) * W];
    }
    float pa[4][5], pb[4][5];
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
        for (int c = 0; c < 5; c++) {
            pa[q][c] = Mc[c * plane + (size_t)min(q + m, H - 1) * W];
            pb[q][c] = Mc[c * plane + (size_t)max(q - m - 1, 0) * W];
        }

    for (int y = 0; y < H; y += 4) {
        float na[4][5], nb[4][5];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int c = 0; c < 5; c++) {
                na[q][c] = Mc[c * plane + (size_t)min(y + 4 + q + m, H - 1) * W];
                nb[q][c] = Mc[c * plane + (size_t)max(y + 4 + q - m - 1, 0) * W];
            }
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int c = 0; c < 5; c++) {
                const float d = pa[q][c] - pb[q][c];
                vs[c] += (double)d;
                sv[q][c][tid] = vs[c];
            }
        __syncthreads();
        const int yo = y + wave, xo = x0 + 4 * lane;
        if (4 * lane < SW && yo < H && xo < W) {
            double g[5];
            float2 o[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                if (p == 0) {
#pragma unroll
                    for (int c = 0; c < 5; c++) {
                        double s = 0;
                        for (int j = 0; j <= 2 * m; j++) s += sv[wave][c][4 * lane + j];
                        g[c] = s;
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 5; c++)
                        g[c] += sv[wave][c][4 * lane + p + 2 * m] - sv[wave][c][4 * lane + p - 1];
                }
                o[p] = nsof_flow_solve(g[0], g[1], g[2], g[3], g[4], scale);
            }
            float2* dst = fz + (size_t)yo * W + xo;
#pragma unroll
            for (int p = 0; p < 4; p++)
                if (4 * lane + p < SW && xo + p < W) dst[p] = o[p];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int c = 0; c < 5; c++) {
                pa[q][c] = na[q][c];
                pb[q][c] = nb[q][c];
            }
    }
}

// ---------------------------------------------------------------------------------------
// FarnebackUpdateFlow_Blur in the reference library's EXACT summation order (NSOF_OPT_EXACT_ROWSUMS).
//
// The library forms the (2m+1)-wide ROW sums as ONE running sum along the whole image row, in double:
// g += vsum[x+m] - vsum[x-m-1] for x = 0..W-1.  The production kernels sum each pixel's window directly -- the same
// numbers to about 1e-16 relative.  Where the 2x2 system is rank deficient (straight edges, flat areas: g11*g22 -
// g12^2 cancels down to the 1e-3 regulariser) those last bits decide the flow's 4th decimal, so on real footage a few
// pixels per frame differ from the library by 1e-4..1e-3.  This pair of kernels reproduces the
// library's order bit for bit at roughly half the speed: the column sums go to HBM (transposed, 40 B/px) and a
// thread walks each image row from left to right.
// ---------------------------------------------------------------------------------------
// thread <-> column: vertical running sums of the 5 planes of M -> VT [n][5][W][H] (transposed: row index fastest)
__global__ __launch_bounds__(256) void k_blur_colsum(const float* __restrict__ M, int W, int H, int m,
                                                      double* __restrict__ VT)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    const size_t plane = (size_t)W * H;
    const float* Mc = M + (size_t)blockIdx.z * 5 * plane + x;
    double* V = VT + (size_t)blockIdx.z * 5 * plane + (size_t)x * H;
    double vs[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        vs[c] = (double)(Mc[c * plane] * (float)(m + 2));   // float product, as "srow0[x]*(m+2)"
        for (int y = 1; y < m; y++) vs[c] += (double)Mc[c * plane + (size_t)min(y, H - 1) * W];
    }
    for (int y = 0; y < H; y++) {
        const size_t ra = (size_t)min(y + m, H - 1) * W, rb = (size_t)max(y - m - 1, 0) * W;
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const float d = Mc[c * plane + ra] - Mc[c * plane + rb];   // rounded to float before it is added
            vs[c] += (double)d;
            V[c * plane + y] = vs[c];
        }
    }
}

// thread <-> row: the library's running row sums + the 2x2 solve, left to right
__global__ __launch_bounds__(64) void k_blur_rowsolve(const double* __restrict__ VT, int W, int H, int m, int block_size,
                                                       float* __restrict__ flow)
{
    const int y = blockIdx.x * 64 + threadIdx.x;
    if (y >= H) return;
    const size_t plane = (size_t)W * H;
    const double* V = VT + (size_t)blockIdx.z * 5 * plane + y;          // V[c*plane + x*H]
    float2* fz = reinterpret_cast<float2*>(flow) + (size_t)blockIdx.z * plane + (size_t)y * W;
    const double scale = 1. / (block_size * block_size);
    auto at = [&](int c, int x) { return V[c * plane + (size_t)clampi(x, 0, W - 1) * H]; };
    double g[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        g[c] = at(c, 0) * (m + 2);
        for (int x = 1; x < m; x++) g[c] += at(c, x);
    }
    for (int x = 0; x < W; x++) {
#pragma unroll
        for (int c = 0; c < 5; c++) g[c] += at(c, x + m) - at(c, x - m - 1);
        fz[x] = nsof_flow_solve(g[0], g[1], g[2], g[3], g[4], scale);
    }
}

}  // namespace

int nsof_launch_blur_solve(nsof_ctx* ctx, int n_pairs, const float* M, int W, int H, int winsize, float* flow)
{
    const int m = winsize / 2;
    if (m > 96) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "winsize=%d too large (max 193)", winsize);
    nsof_prof_scope ps(ctx, NSOF_K_BLUR);
    const int SW = (256 - 2 * m) & ~3;
    dim3 grid((W + SW - 1) / SW, 1, n_pairs);
    hipLaunchKernelGGL(k_blur_solve, grid, dim3(256), 0, ctx->stream, M, W, H, m, winsize, flow);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

int nsof_launch_blur_solve_exact(nsof_ctx* ctx, int n_pairs, const float* M, int W, int H, int winsize, double* VT,
                                 float* flow)
{
    const int m = winsize / 2;
    nsof_prof_scope ps(ctx, NSOF_K_BLUR);
    hipLaunchKernelGGL(k_blur_colsum, dim3((W + 255) / 256, 1, n_pairs), dim3(256), 0, ctx->stream, M, W, H, m, VT);
    hipLaunchKernelGGL(k_blur_rowsolve, dim3((H + 63) / 64, 1, n_pairs), dim3(64), 0, ctx->stream, VT, W, H, m, winsize,
                       flow);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
