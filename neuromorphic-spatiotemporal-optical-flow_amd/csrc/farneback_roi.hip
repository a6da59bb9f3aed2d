// The gated ROI sequence (nsof_farneback_px_roi_sequence_dev): the crops of a gated frame sequence as ONE work list of the
// driver in farneback_batch.hip, and the ordered paste of the crops that overlap an earlier crop of their pair.
#include <algorithm>
#include <cstring>
#include <vector>

#include "nsof_internal.h"

// Whether the rectangle a = (x0, y0, x1, y1) is not empty and meets the rectangle b.
__host__ __device__ static inline bool rect_meets(int ax0, int ay0, int ax1, int ay1, int bx0, int by0, int bx1, int by1)
{
    return ax1 > ax0 && ay1 > ay0 && ax0 < bx1 && bx0 < ax1 && ay0 < by1 && by0 < ay1;
}

// Ordered paste of the private crop fields of nsof_farneback_px_roi_sequence_dev in ONE launch.  The reference's loop pastes
// a pair's crops one after the other, so where extended component boxes overlap the later component wins
// (optical_flow_seg.py:162).  A crop that overlaps an earlier one is computed into a private field; its pixels go to the
// canvas unless a LATER rectangle of the same gating frame covers them (that crop, private by construction, brings its own
// value): every canvas pixel then has exactly one writer among the pastes and the order is the reference's.  The sparse
// config-3 stream has 4425 such crops per 30 frames: as hipMemcpy2DAsync calls they were 12 ms of a 17 ms flow stage.
struct PasteRec {
    float* dst;                   // canvas position of the crop's first vector
    unsigned long long tmp_off;   // float offset of the private field in roi_tmp
    int x0, y0, w, h;
    int frame, idx;               // gating frame and the crop's index in its rectangle list
};
__global__ __launch_bounds__(256) void k_paste_ordered(const PasteRec* __restrict__ recs, const float* __restrict__ tmp,
                                                        const int32_t* __restrict__ counts, const int32_t* __restrict__ rects,
                                                        int max_rects, size_t canvas_pitch)
{
    __shared__ int4 later[256];
    __shared__ int n_later;
    const PasteRec r = recs[blockIdx.z];
    const int area = r.w * r.h;
    if ((int)(blockIdx.x * 1024) >= area) return;   // block-uniform
    const int cnt = min(counts[r.frame], max_rects);
    const int32_t* fr = rects + (size_t)r.frame * max_rects * 4;
    // the later rectangles that touch this crop at all (usually a handful)
    if (threadIdx.x == 0) n_later = 0;
    __syncthreads();
    for (int j = r.idx + 1 + (int)threadIdx.x; j < cnt; j += 256) {
        const int4 q = make_int4(fr[4 * j], fr[4 * j + 1], fr[4 * j + 2], fr[4 * j + 3]);
        if (rect_meets(q.x, q.y, q.z, q.w, r.x0, r.y0, r.x0 + r.w, r.y0 + r.h)) {
            const int k = atomicAdd(&n_later, 1);
            if (k < 256) later[k] = q;
        }
    }
    __syncthreads();
    // more than the LDS list holds: test every later rectangle of the table instead (dropping some would leave pixels
    // with two writers)
    const bool in_lds = n_later <= 256;
    const int nl = in_lds ? n_later : 0;
    const float2* src = reinterpret_cast<const float2*>(tmp + r.tmp_off);
    float2* dst = reinterpret_cast<float2*>(r.dst);
    for (int i = blockIdx.x * 1024 + threadIdx.x; i < min(area, (int)(blockIdx.x + 1) * 1024); i += 256) {
        const int yy = i / r.w, xx = i - yy * r.w;
        const int X = r.x0 + xx, Y = r.y0 + yy;
        bool covered = false;
        for (int k = 0; k < nl && !covered; k++) covered = X >= later[k].x && X < later[k].z && Y >= later[k].y && Y < later[k].w;
        for (int j = r.idx + 1; !in_lds && j < cnt && !covered; j++)
            covered = X >= fr[4 * j] && Y >= fr[4 * j + 1] && X < fr[4 * j + 2] && Y < fr[4 * j + 3];
        if (!covered) dst[(size_t)yy * canvas_pitch + xx] = src[i];
    }
}

namespace {

// The work list of a rectangle table: one item per crop, the pastes of the crops that are computed into a private field,
// and where those fields lie in roi_tmp.
struct RoiList {
    std::vector<nsof_pair_desc> descs;
    std::vector<PasteRec> pastes;
    std::vector<size_t> tmp_slot;   // index into descs of the items whose flow pointer is a roi_tmp offset
    size_t tmp_floats = 0;
    long long pixels = 0;
};

// Rectangle table (host copies of counts and rects) to work list: every non-empty rectangle of the gating frame of every
// pair becomes one item that writes into the pair's canvas in place, or, where it overlaps an earlier rectangle of its
// frame, into a private field (an offset into roi_tmp for now: the buffer may still move) with a paste record.
int roi_work_list(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride, int width,
                  int height, const std::vector<int32_t>& counts, const std::vector<int32_t>& rects, int max_rects, float* d_flows,
                  size_t px, int gate_frame, RoiList* out)
{
    const size_t canvas = (size_t)width * height * 2;   // floats per pair
    for (int k = 0; k + 1 < n_frames; k++) {
        const int cnt = counts[k + gate_frame];
        if (cnt < 0 || cnt > max_rects)
            return nsof_set_error(ctx, NSOF_EINVAL, "roi_sequence: frame %d has %d rectangles, the table holds %d", k + gate_frame, cnt, max_rects);
        const int32_t* r = rects.data() + (size_t)(k + gate_frame) * max_rects * 4;
        for (int i = 0; i < cnt; i++) {
            const int x0 = r[4 * i], y0 = r[4 * i + 1], x1 = r[4 * i + 2], y1 = r[4 * i + 3];
            if (x1 <= x0 || y1 <= y0) continue;
            if (x0 < 0 || y0 < 0 || x1 > width || y1 > height)
                return nsof_set_error(ctx, NSOF_EINVAL, "roi_sequence: rectangle (%d,%d,%d,%d) leaves the %dx%d frame", x0, y0, x1, y1, width, height);
            bool overlap = false;
            for (int j = 0; j < i && !overlap; j++) overlap = rect_meets(r[4 * j], r[4 * j + 1], r[4 * j + 2], r[4 * j + 3], x0, y0, x1, y1);
            nsof_pair_desc d;
            d.prev = d_frames + (size_t)k * frame_stride + (size_t)y0 * row_stride + x0 * px;
            d.next = d_frames + (size_t)(k + 1) * frame_stride + (size_t)y0 * row_stride + x0 * px;
            d.prev_stride = d.next_stride = row_stride;
            d.width = x1 - x0;
            d.height = y1 - y0;
            float* inplace = d_flows + (size_t)k * canvas + ((size_t)y0 * width + x0) * 2;
            if (overlap) {
                out->tmp_slot.push_back(out->descs.size());
                out->pastes.push_back(PasteRec{inplace, (unsigned long long)out->tmp_floats, x0, y0, d.width, d.height, k + gate_frame, i});
                d.flow = reinterpret_cast<float*>(out->tmp_floats * 4);
                d.flow_stride = (ptrdiff_t)d.width * 8;
                out->tmp_floats += (size_t)d.width * d.height * 2;
            } else {
                d.flow = inplace;
                d.flow_stride = (ptrdiff_t)width * 8;
            }
            out->pixels += (long long)d.width * d.height;
            out->descs.push_back(d);
        }
    }
    return NSOF_OK;
}

// Runs a work list (its private fields placed in roi_tmp first) and pastes those fields in order.
int run_and_paste(nsof_ctx* ctx, RoiList& l, int width, const int32_t* d_counts, const int32_t* d_rects, int max_rects,
                  const nsof_list_params& p)
{
    if (l.tmp_floats) {
        if (int rc = ctx->roi_tmp.reserve(ctx, l.tmp_floats * 4)) return rc;
        for (size_t i : l.tmp_slot)
            l.descs[i].flow = reinterpret_cast<float*>((char*)ctx->roi_tmp.p + reinterpret_cast<uintptr_t>(l.descs[i].flow));
    }
    for (size_t i = 0; i < l.descs.size(); i += 32767) {
        const int n = (int)std::min<size_t>(32767, l.descs.size() - i);
        if (int rc = nsof_farneback_list_core(ctx, n, l.descs.data() + i, p)) return rc;
    }
    if (l.pastes.empty()) return NSOF_OK;
    const size_t bytes = l.pastes.size() * sizeof(PasteRec);
    if (int rc = ctx->paste.stage(ctx, bytes, align_up(bytes + bytes / 2, 4096))) return rc;
    memcpy(ctx->paste.h.p, l.pastes.data(), bytes);
    const PasteRec* d_pastes = (const PasteRec*)ctx->paste.upload(ctx, bytes);
    if (!d_pastes) return NSOF_EDEVICE;
    int max_area = 0;
    for (const PasteRec& q : l.pastes) max_area = std::max(max_area, q.w * q.h);
    for (size_t i = 0; i < l.pastes.size(); i += 65535) {
        const unsigned n = (unsigned)std::min<size_t>(65535, l.pastes.size() - i);
        hipLaunchKernelGGL(k_paste_ordered, dim3((unsigned)((max_area + 1023) / 1024), 1, n), dim3(256), 0, ctx->stream,
                           d_pastes + i, (const float*)ctx->roi_tmp.p, d_counts, d_rects, max_rects, (size_t)width);
    }
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

// Gated sequence on the device: frames [n_frames][height] rows of row_stride bytes, the ROI table of the gating kernel
// (nsof_roi_from_surface_dev: counts [n_frames], rects [n_frames][max_rects][4] = x0, y0, x1, y1), flow canvases
// [n_frames - 1][height][width][2].  Pair k = (frame k, frame k + 1) is gated by the rectangles of frame k + gate_frame:
// gate_frame 1 = the map of the pair's SECOND frame, what opticalFlow3D is written to use (memimg2, optical_flow_seg.py:211-252);
// gate_frame 0 = the map of its FIRST frame, what the shipped scripts actually pass (memimg2 := memimg1, optical_flow_seg.py:435;
// the bug-compatible default of nsof.gating).  Every crop of every pair becomes one work item, results land in the zeroed
// canvases in place; a crop that overlaps an earlier crop of its pair (FLAG 1, extended component boxes) is computed into
// a private buffer and pasted afterwards, in label order, as the reference's loop overwrites.  The only traffic over
// PCIe is the rectangle table (16 bytes per ROI): the work list's shapes are needed on the host.
// p.src: the frames' pixel type (the crops' byte addresses, the layout rule and the row stride check follow its size).
int roi_sequence(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride, int width,
                 int height, const int32_t* d_counts, const int32_t* d_rects, int max_rects, float* d_flows,
                 const nsof_list_params& p, int gate_frame, long long* n_calls, long long* n_pixels)
{
    if (!d_frames || !d_counts || !d_rects || !d_flows || n_frames < 2 || max_rects < 1 || width < 1 || height < 1 ||
        !nsof_row_stride_holds(row_stride, width, p.src) || (gate_frame != 0 && gate_frame != 1))
        return nsof_set_error(ctx, NSOF_EINVAL, "roi_sequence: bad argument");
    if (int rc = nsof_check_frame_layout(ctx, p.src, d_frames, row_stride, frame_stride, width, "roi_sequence: d_frames")) return rc;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    NSOF_HIP(ctx, hipMemsetAsync(d_flows, 0, (size_t)(n_frames - 1) * width * height * 8, ctx->stream));
    std::vector<int32_t> counts(n_frames), rects((size_t)n_frames * max_rects * 4);
    NSOF_HIP(ctx, hipMemcpyAsync(counts.data(), d_counts, counts.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipMemcpyAsync(rects.data(), d_rects, rects.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RoiList list;
    if (int rc = roi_work_list(ctx, n_frames, d_frames, row_stride, frame_stride, width, height, counts, rects, max_rects, d_flows, p.px(),
                               gate_frame, &list)) return rc;
    if (n_calls) *n_calls = (long long)list.descs.size();
    if (n_pixels) *n_pixels = list.pixels;
    if (list.descs.empty()) return NSOF_OK;
    return run_and_paste(ctx, list, width, d_counts, d_rects, max_rects, p);
}

}  // namespace

extern "C" int nsof_farneback_px_roi_sequence_dev(nsof_ctx* ctx, int pixel_type, int n_frames, const void* d_frames,
                                                  ptrdiff_t row_stride, ptrdiff_t frame_stride, int width, int height,
                                                  const int32_t* d_counts, const int32_t* d_rects, int max_rects, float* d_flows,
                                                  double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                                                  double poly_sigma, int flags, int gate_frame, long long* n_calls,
                                                  long long* n_pixels)
{
    if (int rc = nsof_check_typed(ctx, pixel_type)) return rc;
    const nsof_list_params p(pixel_type, {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags});
    return roi_sequence(ctx, n_frames, static_cast<const uint8_t*>(d_frames), row_stride, frame_stride, width, height,
                        d_counts, d_rects, max_rects, d_flows, p, gate_frame, n_calls, n_pixels);
}

// ---- the 8-bit and float32 exports of this route: the typed entry with the pixel type named -----------------------------
extern "C" int nsof_farneback_u8_roi_sequence_dev(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames, ptrdiff_t row_stride,
                                                  ptrdiff_t frame_stride, int width, int height, const int32_t* d_counts,
                                                  const int32_t* d_rects, int max_rects, float* d_flows, double pyr_scale,
                                                  int levels, int winsize, int iterations, int poly_n, double poly_sigma,
                                                  int flags, int gate_frame, long long* n_calls, long long* n_pixels)
{
    return nsof_farneback_px_roi_sequence_dev(ctx, NSOF_PIXEL_U8, n_frames, d_frames, row_stride, frame_stride, width, height,
                                              d_counts, d_rects, max_rects, d_flows, pyr_scale, levels, winsize, iterations,
                                              poly_n, poly_sigma, flags, gate_frame, n_calls, n_pixels);
}

extern "C" int nsof_farneback_f32_roi_sequence_dev(nsof_ctx* ctx, int n_frames, const float* d_frames, ptrdiff_t row_stride,
                                                   ptrdiff_t frame_stride, int width, int height, const int32_t* d_counts,
                                                   const int32_t* d_rects, int max_rects, float* d_flows, double pyr_scale,
                                                   int levels, int winsize, int iterations, int poly_n, double poly_sigma,
                                                   int flags, int gate_frame, long long* n_calls, long long* n_pixels)
{
    return nsof_farneback_px_roi_sequence_dev(ctx, NSOF_PIXEL_F32, n_frames, d_frames, row_stride, frame_stride, width, height,
                                              d_counts, d_rects, max_rects, d_flows, pyr_scale, levels, winsize, iterations,
                                              poly_n, poly_sigma, flags, gate_frame, n_calls, n_pixels);
}
