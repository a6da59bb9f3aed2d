// Frame preparation of the frame-driven accumulator on the device: compress_image of
// simulation/simulationcode_v4_transistor_uav.m:111-121 -- imresize(im2double(frame), [out_h out_w], 'lanczos3') -- for a
// stack of 8-bit frames in HBM, in the arithmetic of the host mirror (nsof/frames.py), order included: the result equals
// frames.imresize_lanczos3(im2double(frame), out_h, out_w) bit for bit when the caller passes the mirror's tables.
//
// Order contract.  im2double is double(v) / 255.0 (a 256-entry table formed on the host).  The axis with the smaller
// scale is resized first, rows first on a tie.  Every output sample starts at 0.0 and takes its taps left to right,
// acc = acc + w[k] * v[k], the product rounded before the sum; the intermediate between the two passes is float64.
//
// Kernel shape.  One thread per (frame, output index, position on the other axis): the taps of one output are one
// dependent chain (499 of them at 1080 -> 13), the outputs are independent.
//   k_resize_rows  the row axis: a workgroup is 256 consecutive columns of ONE output row of one frame, so the tap
//                  weights and source rows are uniform over the workgroup (scalar loads) and every tap is one coalesced
//                  row segment.
//   k_resize_cols  the column axis: a workgroup (one wavefront) is 64 consecutive rows of ONE output column.  The
//                  taps of that column are staged through LDS 32 at a time -- 32 neighbouring columns of two rows per
//                  load, never a walk down a column with strided loads -- and every lane then takes its row's 32
//                  samples from LDS in tap order.
// Source indices come mirrored from the host table and are checked there against the axis length before any launch.
#include <cmath>
#include <cstring>

#include "nsof_internal.h"

namespace {

constexpr int ROWS_BLOCK = 256;   // k_resize_rows: columns per workgroup
constexpr int COLS_ROWS = 64;     // k_resize_cols: rows per workgroup (one per lane)
constexpr int COLS_TAPS = 32;     // ... and taps staged per round
constexpr int COLS_PITCH = COLS_TAPS + 1;   // doubles per staged row: lanes r, r+1 start two banks apart (ds_read_b64)

// A source sample as a double: an 8-bit pixel through the im2double table, the float64 intermediate as it is.
__device__ __forceinline__ double sample(const uint8_t* p, ptrdiff_t i, const double* lut) { return lut[p[i]]; }
__device__ __forceinline__ double sample(const double* p, ptrdiff_t i, const double*) { return p[i]; }

// out[f][o][x] = sum over k, in order, of wts[o][k] * src[f][ind[o][k]][x].  Strides in elements of T; out is dense
// [n_frames][out_len][width].  Grid: n_frames * out_len * x_tiles workgroups.
template <class T>
__global__ __launch_bounds__(ROWS_BLOCK) void k_resize_rows(const T* __restrict__ src, ptrdiff_t row_stride,
                                                             ptrdiff_t frame_stride, int width, int out_len,
                                                             const double* __restrict__ wts, const int32_t* __restrict__ ind,
                                                             int taps, const double* __restrict__ lut_g,
                                                             double* __restrict__ out, unsigned x_tiles)
{
    __shared__ double lut[256];
    if (sizeof(T) == 1) {
        lut[threadIdx.x] = lut_g[threadIdx.x];
        __syncthreads();
    }
    const unsigned tile = blockIdx.x % x_tiles, fo = blockIdx.x / x_tiles;
    const unsigned o = fo % (unsigned)out_len, f = fo / (unsigned)out_len;
    const int x = (int)(tile * ROWS_BLOCK + threadIdx.x);
    if (x >= width) return;
    const T* p = src + (ptrdiff_t)f * frame_stride + x;
    const double* w = wts + (size_t)o * taps;
    const int32_t* id = ind + (size_t)o * taps;
    double acc = 0.0;
    for (int k = 0; k < taps; k++) acc = __dadd_rn(acc, __dmul_rn(w[k], sample(p, (ptrdiff_t)id[k] * row_stride, lut)));
    out[((size_t)f * out_len + o) * width + x] = acc;
}

// out[f][y][o] = sum over k, in order, of wts[o][k] * src[f][y][ind[o][k]].  Strides in elements of T; out is dense
// [n_frames][height][out_len].  Grid: n_frames * out_len * y_tiles workgroups of one wavefront.
template <class T>
__global__ __launch_bounds__(COLS_ROWS) void k_resize_cols(const T* __restrict__ src, ptrdiff_t row_stride,
                                                            ptrdiff_t frame_stride, int height, int out_len,
                                                            const double* __restrict__ wts, const int32_t* __restrict__ ind,
                                                            int taps, const double* __restrict__ lut_g,
                                                            double* __restrict__ out, unsigned y_tiles)
{
    __shared__ double lut[256];
    __shared__ double tile[COLS_ROWS * COLS_PITCH];
    if (sizeof(T) == 1)
        for (int i = threadIdx.x; i < 256; i += COLS_ROWS) lut[i] = lut_g[i];
    const unsigned ty = blockIdx.x % y_tiles, fo = blockIdx.x / y_tiles;
    const unsigned o = fo % (unsigned)out_len, f = fo / (unsigned)out_len;
    const int y0 = (int)(ty * COLS_ROWS), lane = (int)threadIdx.x;
    const T* p = src + (ptrdiff_t)f * frame_stride;
    const double* w = wts + (size_t)o * taps;
    const int32_t* id = ind + (size_t)o * taps;
    const int c = lane % COLS_TAPS, r0 = lane / COLS_TAPS;   // staging role: tap c of rows r0, r0 + 2, ...
    double acc = 0.0;
    for (int k0 = 0; k0 < taps; k0 += COLS_TAPS) {
        __syncthreads();   // the table (first round) is written, the previous round's samples are consumed
        const int n = taps - k0 < COLS_TAPS ? taps - k0 : COLS_TAPS;
        if (c < n) {
            const ptrdiff_t col = id[k0 + c];
            for (int r = r0; r < COLS_ROWS && y0 + r < height; r += COLS_ROWS / COLS_TAPS)
                tile[r * COLS_PITCH + c] = sample(p, (ptrdiff_t)(y0 + r) * row_stride + col, lut);
        }
        __syncthreads();
        if (y0 + lane < height)
            for (int k = 0; k < n; k++) acc = __dadd_rn(acc, __dmul_rn(w[k0 + k], tile[lane * COLS_PITCH + k]));
    }
    if (y0 + lane < height) out[((size_t)f * height + (y0 + lane)) * out_len + o] = acc;
}

template <class T>
int launch_rows(nsof_ctx* ctx, int n_frames, const T* src, ptrdiff_t row_stride, ptrdiff_t frame_stride, int width,
                int out_len, const double* wts, const int32_t* ind, int taps, const double* lut, double* out)
{
    const unsigned x_tiles = (unsigned)((width + ROWS_BLOCK - 1) / ROWS_BLOCK);
    const unsigned blocks = (unsigned)n_frames * (unsigned)out_len * x_tiles;   // launch_fits() said so
    hipLaunchKernelGGL(k_resize_rows<T>, dim3(blocks), dim3(ROWS_BLOCK), 0, ctx->stream, src, row_stride, frame_stride,
                       width, out_len, wts, ind, taps, lut, out, x_tiles);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

template <class T>
int launch_cols(nsof_ctx* ctx, int n_frames, const T* src, ptrdiff_t row_stride, ptrdiff_t frame_stride, int height,
                int out_len, const double* wts, const int32_t* ind, int taps, const double* lut, double* out)
{
    const unsigned y_tiles = (unsigned)((height + COLS_ROWS - 1) / COLS_ROWS);
    const unsigned blocks = (unsigned)n_frames * (unsigned)out_len * y_tiles;
    hipLaunchKernelGGL(k_resize_cols<T>, dim3(blocks), dim3(COLS_ROWS), 0, ctx->stream, src, row_stride, frame_stride,
                       height, out_len, wts, ind, taps, lut, out, y_tiles);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// One launch holds a pass when grid x threads stays below 2^32: `other` is the length of the axis that is not resized.
bool launch_fits(int n_frames, int out_len, int other, int per_block)
{
    const unsigned long long tiles = ((unsigned long long)other + per_block - 1) / per_block;
    return (unsigned long long)n_frames * out_len * tiles * per_block <= 0xffffffffull;
}

bool indices_inside(const int32_t* ind, size_t n, int len)
{
    for (size_t i = 0; i < n; i++)
        if (ind[i] < 0 || ind[i] >= len) return false;
    return true;
}

double lanczos3(double x)
{
    const double eps = 2.220446049250313e-16;
    const double f = (std::sin(M_PI * x) * std::sin(M_PI * x / 3) + eps) / ((M_PI * M_PI * (x * x) / 3) + eps);
    return std::fabs(x) < 3 ? f : f * 0.0;
}

}   // namespace

// nsof.frames._contributions restated for C callers (host only): the same expressions for u, left and the kept columns.
extern "C" int nsof_lanczos3_contributions(int in_len, int out_len, double* wts, int32_t* ind, int cap_taps, int* taps)
{
    if (in_len < 1 || out_len < 1 || !taps || (wts && !ind)) return NSOF_EINVAL;
    const double scale = (double)out_len / (double)in_len;
    double kernel_width = 6.0;
    if (scale < 1) kernel_width /= scale;
    const int p = (int)std::ceil(kernel_width) + 2;
    std::vector<double> w((size_t)out_len * p);
    std::vector<long long> left(out_len);
    std::vector<char> keep(p, 0);
    for (int o = 0; o < out_len; o++) {
        const double u = (double)(o + 1) / scale + 0.5 * (1 - 1 / scale);
        left[o] = (long long)std::floor(u - kernel_width / 2);
        double sum = 0.0;
        for (int j = 0; j < p; j++) {
            const double t = u - (double)(left[o] + j);
            sum += (w[(size_t)o * p + j] = scale < 1 ? scale * lanczos3(scale * t) : lanczos3(t));
        }
        for (int j = 0; j < p; j++) {
            w[(size_t)o * p + j] /= sum;
            if (w[(size_t)o * p + j] != 0) keep[j] = 1;
        }
    }
    int kept = 0;
    for (int j = 0; j < p; j++) kept += keep[j];
    *taps = kept;
    if (!wts) return NSOF_OK;
    if (cap_taps < kept) return NSOF_EINVAL;
    const long long period = 2ll * in_len;
    for (int o = 0; o < out_len; o++) {
        int k = 0;
        for (int j = 0; j < p; j++) {
            if (!keep[j]) continue;
            long long m = (left[o] + j - 1) % period;   // 1-based source index, mirrored at both ends as often as it takes
            if (m < 0) m += period;
            wts[(size_t)o * kept + k] = w[(size_t)o * p + j];
            ind[(size_t)o * kept + k] = (int32_t)(m < in_len ? m : period - 1 - m);
            k++;
        }
    }
    return NSOF_OK;
}

extern "C" int nsof_frames_compress_u8_dev(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames, ptrdiff_t row_stride,
                                           ptrdiff_t frame_stride, int width, int height, int out_w, int out_h,
                                           const double* wts_y, const int32_t* ind_y, int taps_y, const double* wts_x,
                                           const int32_t* ind_x, int taps_x, double* d_out)
{
    if (!ctx) return NSOF_EINVAL;
    if (!d_frames || !d_out || !wts_y || !ind_y || !wts_x || !ind_x) return nsof_set_error(ctx, NSOF_EINVAL, "null pointer");
    if (n_frames < 1 || taps_y < 1 || taps_x < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "n_frames %d, taps %d / %d: at least 1 each", n_frames, taps_y, taps_x);
    if (width < 1 || height < 1 || out_w < 1 || out_h < 1)
        return nsof_set_error(ctx, NSOF_EINVAL, "empty frame or empty output (%dx%d -> %dx%d)", width, height, out_w, out_h);
    if (out_w > width || out_h > height)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%dx%d -> %dx%d: a scale above 1 is not built", width, height, out_w, out_h);
    if (row_stride < width) return nsof_set_error(ctx, NSOF_EINVAL, "row stride %td < width %d", row_stride, width);
    const size_t ny = (size_t)out_h * taps_y, nx = (size_t)out_w * taps_x;
    if (!indices_inside(ind_y, ny, height) || !indices_inside(ind_x, nx, width))
        return nsof_set_error(ctx, NSOF_EINVAL, "a source index of the tables lies outside the frame");
    const bool rows_first = (long long)out_h * width <= (long long)out_w * height;   // the smaller scale, rows on a tie
    if (!launch_fits(n_frames, out_h, rows_first ? width : out_w, ROWS_BLOCK) ||
        !launch_fits(n_frames, out_w, rows_first ? out_h : height, COLS_ROWS))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "%d frames of %dx%d: too large for one launch per pass", n_frames, width, height);
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    // one table: im2double | row weights | column weights | row indices | column indices, through the pinned copy
    const size_t o_wy = 256 * sizeof(double), o_wx = o_wy + ny * sizeof(double), o_iy = o_wx + nx * sizeof(double);
    const size_t o_ix = o_iy + ny * sizeof(int32_t), bytes = o_ix + nx * sizeof(int32_t);
    int rc = ctx->frames.stage(ctx, bytes, (bytes + bytes / 2 + 4095) & ~(size_t)4095);
    if (rc) return rc;
    const size_t mid = rows_first ? (size_t)out_h * width : (size_t)height * out_w;
    if ((rc = ctx->tmp.reserve(ctx, (size_t)n_frames * mid * sizeof(double)))) return rc;
    char* h = (char*)ctx->frames.h.p;
    for (int v = 0; v < 256; v++) ((double*)h)[v] = (double)v / 255.0;
    memcpy(h + o_wy, wts_y, ny * sizeof(double));
    memcpy(h + o_wx, wts_x, nx * sizeof(double));
    memcpy(h + o_iy, ind_y, ny * sizeof(int32_t));
    memcpy(h + o_ix, ind_x, nx * sizeof(int32_t));
    const char* d = (const char*)ctx->frames.upload(ctx, bytes);
    if (!d) return NSOF_EDEVICE;
    const double *lut = (const double*)d, *d_wy = (const double*)(d + o_wy), *d_wx = (const double*)(d + o_wx);
    const int32_t *d_iy = (const int32_t*)(d + o_iy), *d_ix = (const int32_t*)(d + o_ix);
    double* d_mid = (double*)ctx->tmp.p;
    if (rows_first) {
        if ((rc = launch_rows(ctx, n_frames, d_frames, row_stride, frame_stride, width, out_h, d_wy, d_iy, taps_y, lut, d_mid)))
            return rc;
        return launch_cols(ctx, n_frames, (const double*)d_mid, (ptrdiff_t)width, (ptrdiff_t)out_h * width, out_h, out_w, d_wx,
                           d_ix, taps_x, lut, d_out);
    }
    if ((rc = launch_cols(ctx, n_frames, d_frames, row_stride, frame_stride, height, out_w, d_wx, d_ix, taps_x, lut, d_mid)))
        return rc;
    return launch_rows(ctx, n_frames, (const double*)d_mid, (ptrdiff_t)out_w, (ptrdiff_t)height * out_w, out_w, out_h, d_wy, d_iy,
                       taps_y, lut, d_out);
}
