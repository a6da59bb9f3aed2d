/*
 * nsof.h -- C ABI of libnsof.so, the MI355X (gfx950) neuromorphic optical-flow core.
 *
 * This is the drop-in boundary for the two data-parallel stages of
 * RTCartist/Neuromorphic-Spatiotemporal-Optical-Flow (paths below are relative to the
 * reference checkout):
 *
 *   stage 2  dense Farneback flow -- replaces `cv2.calcOpticalFlowFarneback(prev, next,
 *            None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags)`
 *            called at optical_flow_seg.py:158,203,494, optical_flow_ob.py:225,270,616,
 *            optical_flow_prediction.py:161,206,570, optical_flow_yolo.py:199,244,898
 *            (parameter dict: optical_flow_seg.py:73-81).
 *   stage 1  synaptic accumulator -- replaces update_state / resistance_exp / simulate of
 *            eventsim/event_mem_sim.py:40-57, :60-63, :164-286.
 *
 * Plain C types only; no torch / numpy types cross this boundary.  All entry points
 * return NSOF_OK (0) or a negative nsof_status; nsof_last_error() gives the text.
 * A context owns one device, one HIP stream and a reusable workspace; it is not
 * thread-safe, several contexts may coexist.  There is no CPU fallback: without a
 * usable gfx950 device nsof_create() fails with NSOF_EDEVICE.
 */
#ifndef NSOF_H
#define NSOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSOF_ABI_VERSION 3   /* 2: NSOF_OPT_EXACT_ROWSUMS defaults to 1; option ranges validated.  3: gate_frame argument of
                              * nsof_farneback_u8_roi_sequence_dev, nsof_accum_set_slice_times, NSOF_OPT_DEBUG_FAULT; a lost
                              * hand-over fails the synchronising call */

typedef enum nsof_status {
    NSOF_OK = 0,
    NSOF_EINVAL = -1,       /* bad argument (cv2 would raise cv2.error on its CV_Assert) */
    NSOF_ESHAPE = -2,       /* prev/next shapes differ or are empty */
    NSOF_EDEVICE = -3,      /* HIP runtime / device failure, or no gfx950 device */
    NSOF_ENOMEM = -4,       /* host or device allocation failed */
    NSOF_EUNSUPPORTED = -5  /* parameters outside what is built: flags other than 0 / NSOF_FARNEBACK_GAUSSIAN, winsize 1, ... */
} nsof_status;

typedef struct nsof_ctx nsof_ctx;

/* ---- context ------------------------------------------------------------------------- */
/* device: HIP device ordinal.  *out receives the context. */
int nsof_create(int device, nsof_ctx** out);
void nsof_destroy(nsof_ctx* ctx);
/* Text of the last error on this context (or of the last failed nsof_create if ctx==NULL). */
const char* nsof_last_error(const nsof_ctx* ctx);
int nsof_abi_version(void);
/* Launch on a caller-owned hipStream_t (e.g. torch's current stream); NULL -> own stream. */
int nsof_set_stream(nsof_ctx* ctx, void* hip_stream);
int nsof_synchronize(nsof_ctx* ctx);
/* Options.  NSOF_OPT_POLYEXP_F32 (default 0): 1 = the polynomial-expansion kernel accumulates its horizontal
 * moments in float instead of double -- faster, but NOT the reference library's arithmetic: the flow then differs
 * from the default (exact) path by the end-point error DESIGN.md reports.  Applies to the uniform-shape entry points;
 * the work-list entries always run the exact kernel.  New contexts take the default from the environment
 * variable NSOF_POLYEXP_F32. */
/* NSOF_OPT_EXACT_ROWSUMS (default 1): the box-filter row sums are formed as the reference library forms them, ONE
 * running double-precision sum along each image row (g += vsum[x+m] - vsum[x-m-1]), inside the fused iteration kernel:
 * every stage then keeps the library's operation order and the flow equals a CPU restatement of the library bit for bit
 * on any input (windows up to 15: one kernel per iteration; larger windows: the unfused kernels, same results).
 * 0 = the "fast row sums" mode: each pixel's window is summed directly -- the same numbers to ~1e-16, a few per cent
 * faster; where the 2x2 system is rank deficient (straight edges and flat areas of real footage, small windows) the
 * rounding history decides the flow's 4th decimal and this mode leaves the library by up to ~8e-4.
 * Environment default: NSOF_EXACT_ROWSUMS. */
/* NSOF_OPT_ROW_BANDS (default 0; applies to the fast row-sum mode only, NSOF_OPT_EXACT_ROWSUMS = 0): for SMALL batches
 * (one call per camera frame, the reference's own call pattern).  The
 * fused iteration kernel walks an image strip top to bottom in one workgroup, because the library's column sums are one
 * running sum from row 0; a lone 1080p pair then occupies 8 of 256 compute units.  1 = split every strip into row bands
 * (automatic height; applied from winsize 9 up), >= 4 = bands of that many rows at any window: each band starts its
 * column sums with a direct sum of its first window, which lacks the rounding history of the running sum -- the same
 * class of deviation as the row-sum order above but more frequent: ~1e-5 on textured frames with wide windows, 4th
 * decimal at many pixels with 3x3 / 4x4 windows (docs/HISTORY_r1_r3.md section 5.1 has the soak counts).  Off by default so that a
 * pair's flow does not depend on the batch it was part of.  Values 2 and 3 are rejected.  Environment default:
 * NSOF_ROW_BANDS. */
/* NSOF_OPT_PYR_FMA (default 0): the arithmetic-variant twin of the pyramid stages.  0 = the float Gaussian blur and the
 * bilinear resamples (pyramid levels, flow resize between levels) round every product and every sum, as the library's
 * generic C++ code does; 1 = the same taps in the same order with one fused multiply-add per tap / blend, as an AVX2+FMA3
 * build of the library's vector loops contracts them.  Which of the two a given cv2 wheel executes cannot be pinned in
 * this image (DESIGN.md section 2 states how far the flow moves between them); both equal their CPU restatement
 * (oracle build of the same switch) bit for bit.  Environment default: NSOF_PYR_FMA. */
/* NSOF_OPT_SMALL_BATCH_JOBS (default 64; exact row-sum order only): the fused iteration kernel gives one workgroup a
 * (192-column strip, image) job and walks the image height in it; a call with at most this many jobs -- a lone frame
 * pair (10 jobs at 1920 wide), a few ROI crops: the reference's own call pattern -- leaves most of the 256 compute
 * units idle, so such calls run the SAME arithmetic in the SAME order as three wide kernels per iteration (matrices;
 * column sums, one thread per column and plane; row sums + solve, one thread per row and plane) with the intermediates
 * in HBM: a lone 1920x1080 call 3.9 -> 1.2 ms host to host.  Results are bit-identical either way; the value only moves
 * the switch-over (measured cross-over: 70-80 jobs, scripts/small_batch_crossover.py; 0 = always the fused kernel).
 * Environment default: NSOF_LAT_JOBS. */
/* NSOF_OPT_DEBUG_FAULT (default 0; TEST HOOK, not a mode): the exact-order iteration kernels hand running sums from one
 * workgroup / wave to the next (strip-to-strip carries in k_iterate_x, wave turns in k_lat_colsum); every wait for such a
 * hand-over is bounded, and a wait that runs out makes the call that synchronises next return NSOF_EDEVICE (cv2 raises
 * cv2.error where it fails, optical_flow_seg.py:203 -- a flow field is never handed back from a failed launch).  Bit 0 = strip
 * 0 of item 0 of every k_iterate_x launch withholds its carries, bit 1 = wave 3 of workgroup (0, 0, 0) of every
 * k_lat_colsum launch never passes its turn on: the failure the bounded waits exist for, on demand
 * (tests/test_farneback_gpu.py::test_lost_handover_is_reported). */
enum { NSOF_OPT_POLYEXP_F32 = 1, NSOF_OPT_EXACT_ROWSUMS = 2, NSOF_OPT_ROW_BANDS = 3, NSOF_OPT_PYR_FMA = 4,
       NSOF_OPT_SMALL_BATCH_JOBS = 5, NSOF_OPT_DEBUG_FAULT = 100 };
int nsof_set_option(nsof_ctx* ctx, int option, int value);
int nsof_get_option(const nsof_ctx* ctx, int option, int* value);

/* ---- stage 2: Farneback --------------------------------------------------------------- */
/* Seven routes lead into the library: a lone host pair, a uniform device batch, a device sequence, a host work list, a
 * device work list, the gated ROI sequence and the stage entry nsof_stage_pyr_level.  Each has ONE typed entry
 * (nsof_farneback_px*, nsof_stage_pyr_level_px), documented below, which takes the frames' pixel type -- an
 * nsof_pixel_type -- after the context: frame pointers are `const void*` and EVERY stride is in BYTES whatever the type.
 * The nsof_farneback_u8* and nsof_farneback_f32* entries (and nsof_stage_pyr_level / nsof_stage_pyr_level_f32) are the
 * typed entry with the pixel type named and typed pointers: they forward to it, so U8 and F32 frames run exactly the same
 * code through either, with the same argument checks, flow layout, host staging and synchronisation.
 *
 * Pixel types: the ones cv2 takes natively on this path.  F32 is what cv2 computes on after its convertTo(CV_32F): a float
 * frame holding the values of an 8-bit frame gives the 8-bit flow bit for bit.  Float frames must be finite (the Python
 * layer checks).  16-bit frames (U16: zero-extended, S16: sign-extended; both convert to float exactly) take the 8-bit
 * path's fused pyramid kernels at 2 B/px and give the flow of F32 frames holding the same values, bit for bit, in every
 * mode.  A work list, a batch or a sequence holds one pixel type.
 *
 * Layout rule, one for every route, in terms of the pixel size s (U8 1, U16 / S16 2, F32 4 bytes): frame pointers
 * s-byte aligned, row, pair and frame strides multiples of s, a row stride at least s * width.  Nothing more: crops that
 * start at any element are fine (the pyramid kernels take their vector loads where rows are aligned for them -- 16 bytes
 * for float frames -- and scalar loads elsewhere; the result does not depend on it).  The lone host pair takes ANY row
 * stride for 8-bit frames (its rows are copied) and the stage entry leaves an 8-bit row stride unchecked.  Otherwise a
 * violation, or an unknown pixel type, returns NSOF_EINVAL before anything is launched.  An entry writes no byte outside
 * the logical elements of its outputs, and its results do not depend on memory outside the logical elements of its inputs
 * (row padding, the space between images, whatever lies before and after a buffer: tests/test_bounds_*_gpu.py). */
/* flags, cv2's values.  0: the box window (FarnebackUpdateFlow_Blur).  NSOF_FARNEBACK_GAUSSIAN (256): every iteration
 * weights its window with a separable Gaussian of sigma 0.3 * (winsize / 2) (FarnebackUpdateFlow_GaussianBlur); winsize 2m
 * and 2m + 1 then give the same flow, winsize up to 193.  Such a call runs k_update_matrices + k_gauss_blur_solve per
 * iteration on every route, whatever the context's options; a work list of mixed shapes runs item by item.
 * NSOF_USE_INITIAL_FLOW (4) is not implemented: it, and every other non-zero value, returns NSOF_EUNSUPPORTED before
 * anything is launched. */
enum { NSOF_USE_INITIAL_FLOW = 4, NSOF_FARNEBACK_GAUSSIAN = 256 };

typedef enum nsof_pixel_type {
    NSOF_PIXEL_U8 = 0,
    NSOF_PIXEL_F32 = 1,
    NSOF_PIXEL_U16 = 2,
    NSOF_PIXEL_S16 = 3,
} nsof_pixel_type;

/* The lone host pair.  Same argument meaning and order as cv2.calcOpticalFlowFarneback (see call sites above).
 * prev/next: HOST single-channel images of pixel_type, row strides in bytes (strided ROI views are
 * fine, optical_flow_seg.py:186-187); flow: HOST float32, interleaved (u,v), row stride in
 * bytes.  Pointers are not retained.  Blocks until the flow is in host memory. */
int nsof_farneback_px(nsof_ctx* ctx, int pixel_type,
                      const void* prev, ptrdiff_t prev_stride,
                      const void* next, ptrdiff_t next_stride,
                      int width, int height,
                      float* flow, ptrdiff_t flow_stride,
                      double pyr_scale, int levels, int winsize, int iterations,
                      int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px(ctx, NSOF_PIXEL_U8, ...) */
int nsof_farneback_u8(nsof_ctx* ctx,
                      const uint8_t* prev, ptrdiff_t prev_stride,
                      const uint8_t* next, ptrdiff_t next_stride,
                      int width, int height,
                      float* flow, ptrdiff_t flow_stride,
                      double pyr_scale, int levels, int winsize, int iterations,
                      int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px(ctx, NSOF_PIXEL_F32, ...) */
int nsof_farneback_f32(nsof_ctx* ctx,
                       const float* prev, ptrdiff_t prev_stride,
                       const float* next, ptrdiff_t next_stride,
                       int width, int height,
                       float* flow, ptrdiff_t flow_stride,
                       double pyr_scale, int levels, int winsize, int iterations,
                       int poly_n, double poly_sigma, int flags);

/* The uniform device batch, the device-resident twin of the lone pair: n_pairs frame pairs of one shape already in HBM.
 * d_prev/d_next: DEVICE frames of pixel_type [n_pairs][height][row_stride]; pair_stride in bytes.
 * d_flow: DEVICE float32 [n_pairs][height][width][2] (dense).  Asynchronous on the
 * context's stream. */
int nsof_farneback_px_batch_dev(nsof_ctx* ctx, int pixel_type, int n_pairs,
                                const void* d_prev, const void* d_next,
                                ptrdiff_t row_stride, ptrdiff_t pair_stride,
                                int width, int height, float* d_flow,
                                double pyr_scale, int levels, int winsize, int iterations,
                                int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_batch_dev(ctx, NSOF_PIXEL_U8, ...) */
int nsof_farneback_u8_batch_dev(nsof_ctx* ctx, int n_pairs,
                                const uint8_t* d_prev, const uint8_t* d_next,
                                ptrdiff_t row_stride, ptrdiff_t pair_stride,
                                int width, int height, float* d_flow,
                                double pyr_scale, int levels, int winsize, int iterations,
                                int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_batch_dev(ctx, NSOF_PIXEL_F32, ...) */
int nsof_farneback_f32_batch_dev(nsof_ctx* ctx, int n_pairs,
                                 const float* d_prev, const float* d_next,
                                 ptrdiff_t row_stride, ptrdiff_t pair_stride,
                                 int width, int height, float* d_flow,
                                 double pyr_scale, int levels, int winsize, int iterations,
                                 int poly_n, double poly_sigma, int flags);

/* The device sequence: n_frames consecutive frames already in HBM, d_frames of pixel_type [n_frames][height][row_stride];
 * d_flow float32 [n_frames-1][height][width][2], flow i = (frame i -> frame i+1), exactly what n_frames-1 calls
 * of nsof_farneback_px on consecutive frames give (the reference's seg/ob/prediction loops walk a sequence this
 * way, optical_flow_seg.py:413-496).  Each frame's pyramid levels and polynomial expansion are computed once and
 * shared by the two pairs the frame belongs to.  Asynchronous on the context's stream. */
int nsof_farneback_px_sequence_dev(nsof_ctx* ctx, int pixel_type, int n_frames, const void* d_frames,
                                   ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                   int width, int height, float* d_flow,
                                   double pyr_scale, int levels, int winsize, int iterations,
                                   int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_sequence_dev(ctx, NSOF_PIXEL_U8, ...) */
int nsof_farneback_u8_sequence_dev(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames,
                                   ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                   int width, int height, float* d_flow,
                                   double pyr_scale, int levels, int winsize, int iterations,
                                   int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_sequence_dev(ctx, NSOF_PIXEL_F32, ...) */
int nsof_farneback_f32_sequence_dev(nsof_ctx* ctx, int n_frames, const float* d_frames,
                                    ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                    int width, int height, float* d_flow,
                                    double pyr_scale, int levels, int winsize, int iterations,
                                    int poly_n, double poly_sigma, int flags);

/* One frame pair of a shape-heterogeneous batch: what ONE call of cv2.calcOpticalFlowFarneback(prev_region,
 * next_region, None, **farneback_params) receives and returns in the gated path -- optical_flow_seg.py:129-164
 * (one crop per connected component), :186-203 (the union box), :492-496 (the full frame) -- as plain pointers.
 * flow_stride in bytes (a multiple of 8): a view flow_canvas[y0:y1, x0:x1] of a frame-sized float32 (H,W,2)
 * canvas is written in place, which is the paste of :162 / :204.  The three structs have the same fields in the same
 * order (one layout) and differ in the type their frame pointers name: nsof_pair_desc_px (untyped frames) for the typed
 * entries, nsof_pair_desc (8-bit) and nsof_pair_desc_f32 (float32) for their exports; every stride stays in BYTES. */
typedef struct nsof_pair_desc_px {
    const void* prev;
    ptrdiff_t prev_stride;
    const void* next;
    ptrdiff_t next_stride;
    int width, height;
    float* flow;
    ptrdiff_t flow_stride;
} nsof_pair_desc_px;
typedef struct nsof_pair_desc {
    const uint8_t* prev;
    ptrdiff_t prev_stride;
    const uint8_t* next;
    ptrdiff_t next_stride;
    int width, height;
    float* flow;
    ptrdiff_t flow_stride;
} nsof_pair_desc;
typedef struct nsof_pair_desc_f32 {
    const float* prev;
    ptrdiff_t prev_stride;
    const float* next;
    ptrdiff_t next_stride;
    int width, height;
    float* flow;
    ptrdiff_t flow_stride;
} nsof_pair_desc_f32;

/* The host work list: n_pairs pairs of ANY shapes, one parameter set, one pixel type, HOST memory (pointers are not
 * retained; blocks until every flow field is in host memory).  All pairs share every kernel launch (a work list per
 * pyramid level), so many small ROI calls cost about as much as one; the list is processed in chunks whose upload,
 * compute and download overlap on three streams.  Buffers from nsof_host_alloc() (page-locked) are copied to/from
 * directly, other memory goes through an internal pinned staging buffer.  The layout rule holds per pair (its frame
 * pointers and row strides).  Result per pair == nsof_farneback_px of that pair, bit for bit, in the default
 * mode; with the opt-in modes that depend on the batch (NSOF_OPT_ROW_BANDS in automatic mode picks its band height from the
 * batch size; a uniform list takes the uniform driver, where NSOF_OPT_POLYEXP_F32 applies) only to their tolerance.
 * Items that start aligned for the level-0 pyramid kernel's vector loads (4 bytes for 8-bit, 8 for 16-bit, 16 for float
 * frames) with row strides that are multiples of that and W % 4 == 0, W >= 8 take its vector form, the others its scalar
 * form; the result does not depend on it. */
int nsof_farneback_px_batch(nsof_ctx* ctx, int pixel_type, int n_pairs, const nsof_pair_desc_px* pairs,
                            double pyr_scale, int levels, int winsize, int iterations,
                            int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_batch(ctx, NSOF_PIXEL_U8, ...) */
int nsof_farneback_u8_batch(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc* pairs,
                            double pyr_scale, int levels, int winsize, int iterations,
                            int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_batch(ctx, NSOF_PIXEL_F32, ...) */
int nsof_farneback_f32_batch(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc_f32* pairs,
                             double pyr_scale, int levels, int winsize, int iterations,
                             int poly_n, double poly_sigma, int flags);

/* The device work list, the device-resident twin of the host one: `pairs` is a HOST array whose prev/next/flow are DEVICE
 * addresses (e.g. crops of frames and of flow canvases already in HBM).  At most 32767 pairs per call
 * (NSOF_EUNSUPPORTED beyond).  Asynchronous on the context's stream. */
int nsof_farneback_px_batch_desc_dev(nsof_ctx* ctx, int pixel_type, int n_pairs, const nsof_pair_desc_px* pairs,
                                     double pyr_scale, int levels, int winsize, int iterations,
                                     int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_batch_desc_dev(ctx, NSOF_PIXEL_U8, ...) */
int nsof_farneback_u8_batch_desc_dev(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc* pairs,
                                     double pyr_scale, int levels, int winsize, int iterations,
                                     int poly_n, double poly_sigma, int flags);
/* nsof_farneback_px_batch_desc_dev(ctx, NSOF_PIXEL_F32, ...) */
int nsof_farneback_f32_batch_desc_dev(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc_f32* pairs,
                                      double pyr_scale, int levels, int winsize, int iterations,
                                      int poly_n, double poly_sigma, int flags);

/* The gated path of a whole frame sequence on the device (opticalFlow3D's crop -> flow -> paste loop,
 * /root/reference/optical_flow_seg.py:129-164, 186-204): d_frames = n_frames frames of pixel_type in HBM (row_stride /
 * frame_stride in bytes, under the layout rule), d_counts / d_rects = the
 * ROI table nsof_roi_from_surface_dev wrote (rects [n_frames][max_rects][4] = x0, y0, x1, y1), d_flows =
 * [n_frames - 1][height][width][2] float canvases, zero-filled here.  Pair k = (frame k, frame k + 1) is gated by the
 * rectangles of frame k + gate_frame: 1 = the map of the pair's second frame (what opticalFlow3D is written to use,
 * memimg2), 0 = the map of its first frame (what the shipped scripts pass: memimg2 := memimg1, optical_flow_seg.py:435 --
 * the bug-compatible default of nsof.gating); every crop of every pair is one item of ONE work list, written into the canvas in place;
 * a crop that overlaps an earlier crop of its pair is pasted after it, in label order, as the reference's loop
 * overwrites.  Each crop's flow equals nsof_farneback_px of that crop bit for bit.  Only the rectangle table crosses
 * PCIe (the work list's shapes are needed on the host; the call synchronises the stream once for it).  n_calls /
 * n_pixels (optional) receive the number of crops and their total area.  Asynchronous otherwise. */
int nsof_farneback_px_roi_sequence_dev(nsof_ctx* ctx, int pixel_type, int n_frames, const void* d_frames,
                                       ptrdiff_t row_stride, ptrdiff_t frame_stride, int width, int height,
                                       const int32_t* d_counts, const int32_t* d_rects, int max_rects, float* d_flows,
                                       double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                                       double poly_sigma, int flags, int gate_frame, long long* n_calls,
                                       long long* n_pixels);
/* nsof_farneback_px_roi_sequence_dev(ctx, NSOF_PIXEL_U8, ...) */
int nsof_farneback_u8_roi_sequence_dev(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames, ptrdiff_t row_stride,
                                       ptrdiff_t frame_stride, int width, int height, const int32_t* d_counts,
                                       const int32_t* d_rects, int max_rects, float* d_flows, double pyr_scale, int levels,
                                       int winsize, int iterations, int poly_n, double poly_sigma, int flags,
                                       int gate_frame, long long* n_calls, long long* n_pixels);
/* nsof_farneback_px_roi_sequence_dev(ctx, NSOF_PIXEL_F32, ...) */
int nsof_farneback_f32_roi_sequence_dev(nsof_ctx* ctx, int n_frames, const float* d_frames, ptrdiff_t row_stride,
                                        ptrdiff_t frame_stride, int width, int height, const int32_t* d_counts,
                                        const int32_t* d_rects, int max_rects, float* d_flows, double pyr_scale, int levels,
                                        int winsize, int iterations, int poly_n, double poly_sigma, int flags,
                                        int gate_frame, long long* n_calls, long long* n_pixels);
/* Page-locked host memory for frames / flow fields handed to nsof_farneback_px_batch and its two exports (NULL on
 * failure). */
void* nsof_host_alloc(size_t bytes);
void nsof_host_free(void* p);

/* Geometry helpers (pure host arithmetic, usable without a device: ctx may be NULL). */
int nsof_farneback_effective_levels(int width, int height, double pyr_scale, int levels);
int nsof_farneback_level_size(int width, int height, double pyr_scale, int level,
                              int* level_width, int* level_height, int* blur_ksize, double* blur_sigma);

/* Individual pipeline stages on DEVICE buffers, exposed for stage-level parity tests and
 * for the roofline benchmark.  Layouts: images [n_img][h][w] float32; flow [n_img][h][w][2]
 * float32; M planar [n_img][5][h][w] float32; the polynomial expansion R of ONE image is
 * 5*h*w float32 = [h][w][4] (channels 0..3 interleaved per pixel) followed by [h][w]
 * (channel 4), images back to back. */
/* Pyramid level `level` of n_img frames of any nsof_pixel_type (byte strides, under the layout rule of the Farneback
 * entries). */
int nsof_stage_pyr_level_px(nsof_ctx* ctx, int pixel_type, int n_img, const void* d_src, ptrdiff_t row_stride,
                            ptrdiff_t img_stride, int width, int height, double pyr_scale, int level, float* d_out);
/* nsof_stage_pyr_level_px(ctx, NSOF_PIXEL_U8, ...) */
int nsof_stage_pyr_level(nsof_ctx* ctx, int n_img, const uint8_t* d_src, ptrdiff_t row_stride,
                         ptrdiff_t img_stride, int width, int height, double pyr_scale, int level, float* d_out);
/* nsof_stage_pyr_level_px(ctx, NSOF_PIXEL_F32, ...) */
int nsof_stage_pyr_level_f32(nsof_ctx* ctx, int n_img, const float* d_src, ptrdiff_t row_stride,
                             ptrdiff_t img_stride, int width, int height, double pyr_scale, int level, float* d_out);
int nsof_stage_polyexp(nsof_ctx* ctx, int n_img, const float* d_img, int width, int height,
                       int poly_n, double poly_sigma, float* d_R);
/* Diagnostic: d_out[i] = the reciprocal the 2x2 solves use (rcp + Newton steps + residual correction, without the
 * scaling / fix-up instructions of a general division) and d_ieee[i] = 1.0 / d_x[i] as the compiler divides; the test
 * asserts they are the same bits over the determinants' range. */
int nsof_stage_recip(nsof_ctx* ctx, long long n, const double* d_x, double* d_out, double* d_ieee);
/* n_pairs pairs: R holds [n_pairs][2][5][h][w] (image 0 = prev, 1 = next). */
int nsof_stage_update_matrices(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_flow,
                               int width, int height, float* d_M);
/* Box blur of M + 2x2 solve.  With NSOF_OPT_EXACT_ROWSUMS on (the default) it runs the unfused exact-order pair the
 * driver uses (column sums, then the library's running row sums; scratch of n_pairs*5*w*h doubles from the context's
 * workspace); off, the per-pixel-sum kernel of the fast mode. */
int nsof_stage_blur_solve(nsof_ctx* ctx, int n_pairs, const float* d_M, int width, int height,
                          int winsize, float* d_flow);
/* The same stage with the Gaussian window of NSOF_FARNEBACK_GAUSSIAN (k_gauss_blur_solve): d_M [n_pairs][5][h][w] planar,
 * d_flow [n_pairs][h][w][2] written; winsize 2..193. */
int nsof_stage_gauss_blur_solve(nsof_ctx* ctx, int n_pairs, const float* d_M, int width, int height,
                                int winsize, float* d_flow);
/* One fused Farneback iteration (matrix update + blur + solve): flow_out = step(R, flow_in).  d_flow_in and
 * d_flow_out must not alias.  winsize 2..15; larger windows take the unfused pair above. */
int nsof_stage_iterate(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_flow_in, int width, int height,
                       int winsize, float* d_flow_out);
/* Formerly the same with flow_in = resample(d_coarse_flow [src_h][src_w][2]) * (1/pyr_scale) formed on the fly.
 * That kernel was removed (measured slower than the separate resample); the symbol stays for the ABI: it checks its
 * arguments (NSOF_EINVAL) and otherwise returns NSOF_EUNSUPPORTED. */
int nsof_stage_iterate_upsample(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_coarse_flow,
                                int src_w, int src_h, int width, int height, int winsize, double pyr_scale,
                                float* d_flow_out);
/* One exact-order fused iteration whose flow_in is resample(d_coarse_flow [src_h][src_w][2]) * (1/pyr_scale), formed
 * inside the kernel as its rows are fetched (k_iterate_xr): bit for bit nsof_stage_flow_upsample followed by
 * nsof_stage_iterate in exact mode.  NSOF_EUNSUPPORTED, nothing written, unless width == 2 * src_w,
 * height == 2 * src_h and winsize is 2..15. */
int nsof_stage_iterate_x_resample(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_coarse_flow,
                                  int src_w, int src_h, int width, int height, int winsize, double pyr_scale,
                                  float* d_flow_out);
int nsof_stage_flow_upsample(nsof_ctx* ctx, int n_pairs, const float* d_src, int src_w, int src_h,
                             float* d_dst, int dst_w, int dst_h, double pyr_scale);

/* ---- profiling (HIP events on the context's stream, around every launch of one kernel) -- */
typedef enum nsof_kernel_id {
    NSOF_K_PREP = 0,        /* u8 -> f32, Gaussian blur, bilinear resample (per level) */
    NSOF_K_POLYEXP = 1,     /* polynomial expansion */
    NSOF_K_UPSAMPLE = 2,    /* coarse-to-fine flow resample */
    NSOF_K_UPDMAT = 3,      /* matrix update with warped R1 */
    NSOF_K_BLUR = 4,        /* box blur + 2x2 solve */
    NSOF_K_ACCUM = 5,       /* accumulator state update */
    NSOF_K_ITERATE = 6,     /* fused matrix update + box blur + solve (one Farneback iteration) */
    NSOF_K_SEGMENT = 7,     /* |flow| > th (or u8 != 0) -> bit-packed mask */
    NSOF_K_MORPH = 8,       /* fused dilate/erode chain on the bit-packed mask */
    NSOF_K_REMAP = 9,       /* 8-bit bilinear remap / fused prediction warp */
    NSOF_K_SSIM = 10,       /* SSIM window statistics + per-block partial sums */
    NSOF_K_COUNT = 11
} nsof_kernel_id;
/* mask: bit (1<<id) enables event bracketing for that kernel; 0 disables. */
int nsof_prof_enable(nsof_ctx* ctx, unsigned mask);
/* Synchronises, then returns summed device time (ms) and launch count since the last call. */
int nsof_prof_collect(nsof_ctx* ctx, int kernel_id, double* total_ms, long long* launches);
const char* nsof_kernel_name(int kernel_id);

/* ---- stage 1: synaptic accumulator ---------------------------------------------------- */
typedef struct nsof_accum nsof_accum;

/* Device constants default to event_mem_sim.py:20-34 (PARAMS, DT=5e-4, REFRACTORY_US=800; nsof_accum_create_p takes
 * others); scheme 1's THETA_EVENTS defaults to 1 (nsof_accum_set_event_threshold).  scheme: 1 = boxcar window, 2 = DC bias +
 * event overlay (:208-286).
 * polarity_split: scheme 2 only -- 1 = 'split' (ON p==1 -> array A, OFF p==0 -> array B),
 * 0 = 'magnitude' (one array). */
int nsof_accum_create(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split,
                      float active_v, float silent_v, nsof_accum** out);
/* The device model as an argument, as the reference takes it (update_state(w, V, p=PARAMS, dt=DT), resistance_exp(w,
 * p=PARAMS); REFRACTORY_US is the module knob simulate reads).  The entries above and below that take no parameters are
 * the _p entries with NULL, i.e. with the values nsof_accum_default_params returns (the fitted device of the paper).
 * float32 paths: every field is rounded to float32 once on the host, as NumPy rounds the Python scalars next to a
 * float32 array; dw/dt = (k * (V/v0 - 1) ** alpha) * (1 - w*s) ** b in that order, each power evaluated in double from the
 * float32 operands and rounded once, alpha == 1 calling no power; a base <= 0 or non-finite follows np.power on float32
 * operands (integer exponents keep the sign for odd ones).  float64 frame path: the same fields as doubles.
 * Refused with NSOF_EINVAL before anything is launched: a non-finite field (or one that is not finite as float32),
 * !(voff < 0 < von), son or soff outside [0, 1], Ron <= 0 or Roff <= 0, wini outside [0, 1], dt <= 0, refractory_us < 0.
 * Not a field of this struct: scheme 1's event threshold THETA_EVENTS is a setting of the accumulator
 * (nsof_accum_set_event_threshold).  One device per array unless nsof_accum_set_param_maps hands in per-pixel planes.
 * Per-pixel thresholds and the linear resistance map are not supported. */
typedef struct nsof_accum_params {      /* keys of PARAMS (event_mem_sim.py:20-27); won / woff are read by nothing and not carried */
    double alphaoff, alphaon, voff, von, koff, kon, son, soff, bon, boff, Ron, Roff, wini;
    double dt;                          /* DT, seconds */
    int64_t refractory_us;              /* REFRACTORY_US */
} nsof_accum_params;
void nsof_accum_default_params(nsof_accum_params* out);
/* nsof_accum_create for an array of the given device (params NULL = defaults); the model is fixed for the accumulator's life
 * and every update form, surface, snapshot, block current and reset (w = wini) of it uses it. */
int nsof_accum_create_p(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v, float silent_v,
                        const nsof_accum_params* params, nsof_accum** out);
int nsof_accum_get_params(const nsof_accum* acc, nsof_accum_params* out);
/* Per-pixel parameter maps: an array whose devices differ (fabrication spread in Ron / Roff, thresholds, rate constants,
 * initial state).  keys[j] names a field of nsof_accum_params, maps[j] is its HOST float32 plane [H][W] (not retained).  A
 * mapped key takes the pixel's float32 value, every other key keeps the accumulator's scalar (nsof_accum_get_params keeps
 * returning the scalars); dt, refractory_us, theta and the two voltages stay scalars.  Per pixel the arithmetic is that of
 * the uniform model with the pixel's own float32 fields, neg_lam = (float)(-ln(Roff / Ron)) with the logarithm in double of
 * the values as held (a plane's float32 widened, a scalar's double): constant planes equal to the scalars give the uniform
 * accumulator's bits.  Every update form, surface (u8, f32), snapshot, resistance read-out and block current follows.
 * Accepted only on an accumulator that is fresh or has just been reset (slice counter 0, no snapshots); the call ends with a
 * reset, and from then on nsof_accum_reset sets w to the wini plane where wini is mapped.  n_maps == 0 returns to the
 * uniform model.  Synchronous.
 * NSOF_EINVAL, the accumulator keeping its model and state: a key outside [0, NSOF_ACCUM_KEY_COUNT), a key given twice, a
 * NULL plane, an accumulator that has advanced, and any pixel outside the domain nsof_accum_create_p checks -- non-finite,
 * voff >= 0, von <= 0, son / soff / wini outside [0, 1], Ron or Roff <= 0 -- the message naming the key and the first such
 * pixel (row, column, value).  The check is a host pass over the planes before anything is uploaded.
 * Device form: one set-up kernel per call writes, per pixel, the drive (k * (V/v0 - 1) ** alpha, s, b) at the active and at
 * the silent voltage and the pair (Ron, neg_lam); the update kernels read a pixel's 12-byte drive where they formed one
 * from their arguments.  The dead-zone shortcut (nsof_accum_set_dense) holds when silent_v lies in [voff, von] at EVERY
 * pixel; otherwise every advancing call takes the every-pixel pass with the per-pixel silent drive, whatever force_dense.
 * nsof_accum_run_frames on a mapped accumulator takes copy + patch where it applies and n_frames x nsof_accum_run_surface
 * otherwise; the tile walk has no mapped form and is routed around (nsof_accum_set_frames_path changes nothing then).
 * Out of scope: the element-wise nsof_accum_update_state*_dev / nsof_accum_resistance*_dev entries (one device per call),
 * row-band sharding in nsof/dist.py (a band factory takes no maps), the linear resistance map, per-pixel thresholds.  The
 * float64 frame-driven path has maps of its own: nsof_accum_frames_f64_maps_dev. */
enum {
    NSOF_ACCUM_KEY_ALPHAOFF = 0, NSOF_ACCUM_KEY_ALPHAON, NSOF_ACCUM_KEY_VOFF, NSOF_ACCUM_KEY_VON, NSOF_ACCUM_KEY_KOFF,
    NSOF_ACCUM_KEY_KON, NSOF_ACCUM_KEY_SON, NSOF_ACCUM_KEY_SOFF, NSOF_ACCUM_KEY_BON, NSOF_ACCUM_KEY_BOFF, NSOF_ACCUM_KEY_RON,
    NSOF_ACCUM_KEY_ROFF, NSOF_ACCUM_KEY_WINI, NSOF_ACCUM_KEY_COUNT   /* = 13: the double fields of nsof_accum_params, in order */
};
int nsof_accum_set_param_maps(nsof_accum* acc, int n_maps, const int* keys, const float* const* maps);
/* The plane of a mapped key as it was set, float32 [H][W] to HOST memory; NSOF_EINVAL if that key is uniform. */
int nsof_accum_read_param_map(nsof_accum* acc, int key, float* out);
/* Bit k of *mask set: key k is a map. */
int nsof_accum_param_map_mask(const nsof_accum* acc, unsigned* mask);
void nsof_accum_destroy(nsof_accum* acc);
/* With silent_v in the dead zone an idle pixel is a bit-exact no-op, so two updates give the same state: the event-pixel
 * update (only touched pixels, groups of 32 slices) and the every-pixel pass (scheme 1: groups of 64 slices, no lists).
 * force_dense 0 (default) = automatic: scheme 1 takes the every-pixel pass up to ~12 M pixels (it needs half the launches:
 * 1280x720 0.39 vs 0.75-0.89 ms per 30 surface frames, 3840x2160 0.97 vs 1.21 ms), the event-pixel update beyond and in
 * scheme 2; > 0 = always the every-pixel pass (the roofline run); < 0 = the event-pixel update wherever it is exact. */
int nsof_accum_set_dense(nsof_accum* acc, int force_dense);
/* Scheme 1's THETA_EVENTS (event_mem_sim.py:33, :208-217): a pixel pulses in a slice when at least theta events fall on it in
 * that slice, whatever their polarity; default 1.  A run at theta is the theta == 1 run on the stream without the events of
 * every (pixel, slice) cell that holds fewer than theta events -- every update form, snapshot, surface and frame follows.
 * May be set between any two advancing calls and holds from the next one.  theta == 1 runs the kernels it always ran (one
 * mask bit per slice).  theta > 1: the mask word holds a saturating counter of b = ceil(log2(theta + 1)) bits per slice (a
 * compare-and-swap loop that stops at theta: no count overflows, theta up to INT32_MAX), so a group is 32 / b slices in
 * the event-pixel update and 2 * (32 / b) in the every-pixel pass instead of 32 and 64, and no memory is added.
 * nsof_accum_run_frames with theta > 1 never takes the tile walk: where copy + patch applies (every <= 64) it takes copy +
 * patch, an interval in ceil(every / (64 / b)) rounds of (scatter, update of the touched pixels) on the one 64-bit word per
 * pixel, the first round copying the frame; n_frames x nsof_accum_run_surface otherwise -- the same bytes either way.
 * NSOF_EINVAL, with the value in the message and nothing launched, allocated or changed: theta < 1; theta != 1 on a scheme-2
 * accumulator (the reference records theta_events = None there: the scheme has no count threshold). */
int nsof_accum_set_event_threshold(nsof_accum* acc, int theta);
int nsof_accum_get_event_threshold(const nsof_accum* acc, int* theta);
/* Reset w to the model's wini (default 0.5; the wini plane where one is set) and the refractory maps to 0. */
int nsof_accum_reset(nsof_accum* acc);
/* Advance by n_slices time slices.  Events are HOST arrays (x,y int16; p int8; t int64 us,
 * sorted) as in the /CD/events group (event_mem_sim.py:69-75); slice_bounds has
 * n_slices+1 entries: slice i covers events [slice_bounds[i], slice_bounds[i+1]).  If
 * snap_every > 0, after every slice whose global index (counted since reset) is a multiple
 * of snap_every a resistance snapshot is appended to the snapshot ring. */
int nsof_accum_step_events(nsof_accum* acc, const int16_t* x, const int16_t* y, const int8_t* p,
                           const int64_t* t, const int64_t* slice_bounds, int64_t n_slices,
                           int64_t snap_every);
/* The same in two halves, for streams that are advanced piecewise or re-run: nsof_accum_set_events uploads the
 * events of slices [0, n_slices) ONCE (arrays and bounds as above; nothing is retained but the device copy), and
 * nsof_accum_run advances over any sub-range [first_slice, first_slice + n_slices) of them without touching the
 * host arrays again.  nsof_accum_step_events == set_events followed by run(0, n_slices). */
int nsof_accum_set_events(nsof_accum* acc, const int16_t* x, const int16_t* y, const int8_t* p,
                          const int64_t* t, const int64_t* slice_bounds, int64_t n_slices);
int nsof_accum_run(nsof_accum* acc, int64_t first_slice, int64_t n_slices, int64_t snap_every);
/* nsof_accum_set_events / nsof_accum_step_events for a stream that lies in DEVICE memory -- what
 * nsof_events_from_frames_*_dev and nsof_events_denoise_compact_dev write: d_x, d_y (int16), d_p (int8; may be NULL where
 * the host entry allows it: every case but scheme 2 with polarity_split) and d_t (int64) hold n_events events; slice_bounds
 * is a HOST array of n_slices + 1 indices into them, 0 <= slice_bounds[0] and slice_bounds[n_slices] <= n_events, else
 * NSOF_EINVAL.  The contracts are the host twins': the same refusals with the same messages -- an event outside the sensor
 * is "event %lld at (%d,%d) outside the %dx%d sensor", the first one in stream order -- found by one pass on the device
 * (a wave reduces, then one atomic minimum per wave that found a fault).  A refused call launches nothing that writes the
 * accumulator: state, snapshots and a previously staged stream stay as they were.  After a successful call the state,
 * snapshots, surfaces and frames equal the host entry's on the same stream bit for bit; the caller's arrays are not
 * retained.
 * Stream: the entries work on the context's stream and WAIT for it twice per staged stream: once for the check's verdict
 * (which, for scheme 2, brings every slice's first and last time along: 32 B + 16 B per slice, one copy; 8 B per slice of
 * bounds went up before), and once at the end of the staging, after the events have been copied device to device, so
 * that the caller may free or overwrite its arrays when the call returns.  The events never cross PCIe.  Work that
 * produced the arrays on another stream must have completed before the call. */
int nsof_accum_set_events_dev(nsof_accum* acc, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                              int64_t n_events, const int64_t* slice_bounds, int64_t n_slices);
int nsof_accum_step_events_dev(nsof_accum* acc, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                               int64_t n_events, const int64_t* slice_bounds, int64_t n_slices, int64_t snap_every);
/* Scheme 2 only (a no-op for scheme 1): replace the per-slice timestamps nsof_accum_set_events derived from the staged
 * events -- the first event's time (refractory test) and the last event's (next_ok = t_last + 800 us),
 * event_mem_sim.py:243-267 -- by those of the WHOLE stream's slices.  For an accumulator that holds a row band of the
 * sensor and was staged with the band's events only: its state then equals the band's rows of the unsharded run
 * (SURVEY.md section 8e).  n_slices must equal the staged count; call between set_events and run. */
int nsof_accum_set_slice_times(nsof_accum* acc, const int64_t* t_first, const int64_t* t_last, int64_t n_slices);
/* The current surface as an 8-bit frame on the DEVICE, d_out uint8 [H][row_stride]; asynchronous on the context's
 * stream.  mode NSOF_SURFACE_CURRENT: g = uint8(clip(-3366/log10(I) - 306, 0, 255)), I = 1/R, R = resistance_exp(w) --
 * the reference's map from device current to the gating image (optical_flow_seg.py:426-431) applied per pixel
 * (calibrated for arrays that start at w = 0; the event simulator's initial w = 0.5 already gives 255).
 * mode NSOF_SURFACE_STATE: g = uint8(255 * w), the build-defined frame of the joined events -> flow pipeline. */
enum { NSOF_SURFACE_CURRENT = 0, NSOF_SURFACE_STATE = 1 };
int nsof_accum_surface_u8_dev(nsof_accum* acc, int which, int mode, uint8_t* d_out, ptrdiff_t row_stride);
/* The same surface as a float32 frame on the DEVICE, d_out [H][row_stride_bytes / 4]: g computed as above and clipped to
 * [0, 255], rounded to float instead of truncated to 8 bits (always finite; floor of it is the 8-bit frame's value).  The
 * unquantised input of the float Farneback entries.  Asynchronous on the context's stream. */
int nsof_accum_surface_f32_dev(nsof_accum* acc, int which, int mode, float* d_out, ptrdiff_t row_stride_bytes);
/* nsof_accum_run + nsof_accum_surface_u8_dev of the state after the run's last slice, as one call: where the dense
 * scheme-1 update runs, its last pass writes the frame itself (no separate pass over the array, one launch less); the
 * frame is byte-identical to the two calls. */
int nsof_accum_run_surface(nsof_accum* a, int64_t first_slice, int64_t n_slices, int which, int mode, uint8_t* d_out,
                           ptrdiff_t row_stride);
/* n_frames consecutive intervals of `every` slices, the surface after each interval into d_frames + k * frame_stride (uint8
 * [H][row_stride] each) -- what n_frames calls of nsof_accum_run_surface give, byte for byte, issued from one call.  Scheme 1
 * with the silent voltage in the dead zone [voff, von] (no forced every-pixel pass, every <= 64): frame k is frame k-1 copied
 * (2 B/px) and patched at the pixels the interval's events touched, the state updated at those pixels only -- or, by
 * default, the whole run as one tile-persistent walk (nsof_accum_set_frames_path).  Asynchronous on the context's stream. */
int nsof_accum_run_frames(nsof_accum* acc, int64_t first_slice, int64_t n_frames, int64_t every, int which, int mode,
                          uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride);
/* Which of its two event-driven forms nsof_accum_run_frames takes where both apply (same bytes): 0 (default) = the tile
 * walk -- a wave owns 1024 consecutive pixels for the whole run (state, current frame bytes and slice masks in LDS), the
 * run's events are bucketed by (interval, tile) first, frames are write-only: two launches per call; needs sensor width,
 * row and frame strides that are multiples of 16 and a 16-byte aligned frame buffer -- 1 = copy + patch per interval (two
 * launches per interval; what the tile walk falls back to, and its cross-check in the tests). */
int nsof_accum_set_frames_path(nsof_accum* acc, int path);
/* Checkpoint / resume (the reference persists only w_final, event_mem_sim.py:289-303): copy one array's state to /
 * from HOST memory -- w float32 [H][W], the refractory map int64 [H][W] (scheme 2; zeros otherwise) and the global
 * slice counter that times the snapshots.  NULL pointers are skipped. */
int nsof_accum_read_state(nsof_accum* acc, int which, float* w_out, int64_t* next_ok_out, int64_t* slice_counter);
int nsof_accum_write_state(nsof_accum* acc, int which, const float* w_in, const int64_t* next_ok_in,
                           int64_t slice_counter);
/* Dense element-wise update_state on DEVICE arrays (event_mem_sim.py:40-57). */
int nsof_accum_update_state_dev(nsof_ctx* ctx, const float* d_w, const float* d_V, float* d_out, size_t n);
/* update_state(w, V, p, dt): dt is params->dt. */
int nsof_accum_update_state_p_dev(nsof_ctx* ctx, const nsof_accum_params* params, const float* d_w, const float* d_V,
                                  float* d_out, size_t n);
/* bincount_2d(x, y, H, W) of event_mem_sim.py:100-104: events per pixel, int32 [H][W].  HOST arrays in and out;
 * events outside the sensor are an error (np.bincount would raise or grow the array). */
int nsof_accum_bincount_2d(nsof_ctx* ctx, const int16_t* x, const int16_t* y, size_t n, int height, int width,
                           int32_t* counts_out);
/* Dense resistance_exp on DEVICE arrays (event_mem_sim.py:60-63). */
int nsof_accum_resistance_dev(nsof_ctx* ctx, const float* d_w, float* d_out, size_t n);
/* resistance_exp(w, p). */
int nsof_accum_resistance_p_dev(nsof_ctx* ctx, const nsof_accum_params* params, const float* d_w, float* d_out, size_t n);
/* Copy state to HOST: which = 0 (array A) or 1 (array B, split mode). */
int nsof_accum_read_w(nsof_accum* acc, int which, float* w_out);
int nsof_accum_read_resistance(nsof_accum* acc, int which, float* r_out);
/* Snapshots taken so far; copy them ([count][H][W] float32) to HOST and clear the ring. */
int64_t nsof_accum_snapshot_count(const nsof_accum* acc);
int nsof_accum_read_snapshots(nsof_accum* acc, int which, float* out, int64_t max_count);
/* Input of the gating image formed on the device: out[H/memsize][W/memsize] (HOST, float64) = the maximum of the device
 * current v_ds / R over every memsize x memsize block of pixels -- of stored snapshot `snapshot` (0-based, not consumed), or
 * of the current state when snapshot < 0.  Same values as dividing the downloaded float32 resistance map on the host
 * (max of v_ds/R = v_ds / min R); only rows x cols doubles cross PCIe instead of the whole surface. */
int nsof_accum_block_current(nsof_accum* acc, int which, int64_t snapshot, int memsize, double v_ds, double* out);
/* The same map written to DEVICE memory (d_out: rows x cols doubles), asynchronous on the context's stream: the input of
 * nsof_roi_from_surface_dev. */
int nsof_accum_block_current_dev(nsof_accum* acc, int which, int64_t snapshot, int memsize, double v_ds, double* d_out);
/* Frame-driven variant of the same device ODE (simulation/simulationcode_v4_transistor_uav.m:146-227,332-347),
 * float64: imgs = HOST compressed frames [n_frames][H][W] in [0,1]; per frame pair the drive voltage comes
 * from |a-b|*256 through the piecewise map (th1, th2) and modulatefunc, followed by n_sub_steps Euler sub-steps
 * of dt/n_sub_steps.  w_out [H][W]; res_out [n_frames][H][W] (initial array, then one snapshot per pair).
 * One implementation serves all eight nsof_accum_frames_f64* entries: this one is nsof_accum_frames_f64_maps with one trial and
 * no maps (upload, ONE launch, download; synchronous), so it shares that entry's launch range -- NSOF_EUNSUPPORTED beyond
 * 2^32 - 64 cells, which no real array comes near. */
int nsof_accum_frames_f64(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                          int n_sub_steps, double th1, double th2, double* w_out, double* res_out);
/* simulate_memristor_array(..., params): the same run for the given device (NULL = defaults), the fields read as doubles;
 * the array starts at wini, lambda = ln(Roff / Ron).  dt stays the argument it is: params->dt and params->refractory_us
 * are checked with the rest of the set and not read. */
int nsof_accum_frames_f64_p(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                            int n_sub_steps, double th1, double th2, const nsof_accum_params* params, double* w_out,
                            double* res_out);
/* The same run on DEVICE arrays in ONE launch (one thread per grid pixel walks every frame pair), asynchronous on the
 * context's stream, nothing copied: d_imgs [n_frames][H][W]; d_w [H][W]; d_res [n_frames][H][W], slice 0 the initial array
 * and slice f + 1 the state after pair (f, f + 1); d_current (may be NULL) [n_frames - 1][H][W], d_current[f] = v_ds /
 * d_res[f + 1] as an IEEE double division -- the device current of a grid that already is the gating map, the layout
 * nsof_roi_from_surface_dev reads.  This is nsof_accum_frames_f64_maps_dev with one trial and no maps, except that d_res
 * must be given; the host entries run the same kernel, so d_w and d_res equal their outputs bit for bit, and the bits
 * themselves -- those of the per-pair host entry this kernel replaced -- are recorded in tests/golden/frames_run_bits.npz
 * (tests/test_frames_bits_gpu.py). */
int nsof_accum_frames_f64_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                              int n_sub_steps, double th1, double th2, double v_ds, double* d_w, double* d_res,
                              double* d_current);
int nsof_accum_frames_f64_p_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                                int n_sub_steps, double th1, double th2, double v_ds, const nsof_accum_params* params,
                                double* d_w, double* d_res, double* d_current);
/* The array run with a device model per cell AND per trial: device-to-device variability of the physical gating array, all
 * n_trials Monte-Carlo trials of a study in one launch.  keys[j] names a field of nsof_accum_params (NSOF_ACCUM_KEY_*),
 * planes[j] is its HOST float64 plane (not retained) of plane_trials[j] trials: n_trials ([T][H][W]) or 1 ([H][W], shared by
 * all trials).  A mapped key takes the value of its (trial, cell), every other key the scalar of params (NULL = defaults); dt,
 * th1, th2, v_ds and n_sub_steps stay scalars.  Values are read as doubles (a float32 plane widened is exact).  The frames
 * d_imgs [n_frames][H][W] are shared by the trials; d_w [T][H][W], d_res [T][n_frames][H][W] (may be NULL), d_current
 * [T][n_frames - 1][H][W] (may be NULL), each trial laid out as nsof_accum_frames_f64_dev lays out its one.
 * Every other noiseless nsof_accum_frames_f64* entry ends here, and this one in nsof_accum_frames_f64_c2c_dev (below), the
 * entry that launches, called without noise.  One kernel walks a (trial, cell)'s
 * frame pairs whatever the source of its device model -- the fitted constants, the scalars of params, planes -- so per
 * (trial, cell) the arithmetic is the uniform call's with that cell's fields.  The two values formed on the host with the C
 * library, lambda = log(Roff / Ron) and the initial resistance Ron / exp(-lambda * (1 - wini)), are formed there per (trial,
 * cell) wherever Ron, Roff or wini is a plane, and uploaded as planes.  So a cell's w, res and current equal, bit for bit,
 * nsof_accum_frames_f64_p_dev's at that cell's parameters; constant planes equal to the scalars give the uniform bits; with
 * n_maps == 0 every trial is the uniform run.
 * Thread g of the launch is trial g / (H * W), cell g % (H * W), in workgroups of 64.  The planes go up through a buffer of
 * the context, stream-ordered: the call waits only for its own previous upload to have left the pinned copy, or to grow it;
 * otherwise asynchronous on the context's stream.
 * NSOF_EINVAL, nothing uploaded, launched or written: n_trials < 1, a key outside [0, NSOF_ACCUM_KEY_COUNT) or given twice, a
 * NULL plane, plane_trials[j] other than 1 or n_trials, and any value outside the domain nsof_accum_create_p checks
 * (non-finite as double or as float32, voff >= 0, von <= 0, son / soff / wini outside [0, 1], Ron or Roff <= 0, ln(Roff /
 * Ron) not finite) -- the message naming key, trial, row, column and value of the first one, planes in the order given.
 * NSOF_EUNSUPPORTED (likewise before anything is uploaded): n_trials * H * W beyond one launch's index range, 2^32 - 64.
 * Out of scope: per-cell th1 / th2 / dt, the linear resistance map, float32 planes on the device. */
int nsof_accum_frames_f64_maps_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                                   int n_sub_steps, double th1, double th2, double v_ds, const nsof_accum_params* params,
                                   int n_trials, int n_maps, const int* keys, const double* const* planes,
                                   const int* plane_trials, double* d_w, double* d_res, double* d_current);
/* The same with HOST frames and outputs (w_out [T][H][W], res_out [T][n_frames][H][W]) -- the one host path: validate,
 * upload, the device entry, download, synchronise.  The device entry's bits. */
int nsof_accum_frames_f64_maps(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                               int n_sub_steps, double th1, double th2, const nsof_accum_params* params, int n_trials,
                               int n_maps, const int* keys, const double* const* planes, const int* plane_trials,
                               double* w_out, double* res_out);
/* The EVENT-driven accumulator with a device model per pixel AND per trial: all n_trials Monte-Carlo trials of a
 * device-variability study on one event stream, in one run.  Self-contained like nsof_accum_frames_f64_p_dev: no
 * accumulator object, no resume.  Geometry, scheme, polarity_split, active_v, silent_v and params (NULL = the fitted device)
 * as nsof_accum_create_p takes them, theta as nsof_accum_set_event_threshold (scheme 1 only beyond 1); x, y, p, t,
 * slice_bounds and n_slices (>= 1) are HOST arrays as nsof_accum_step_events takes them (not retained).  keys / planes /
 * plane_trials follow nsof_accum_frames_f64_maps_dev's convention with HOST float32 planes: plane_trials[j] is n_trials
 * ([T][H][W]) or 1 ([H][W], shared by all trials); an unmapped key keeps the scalar of params.
 * Outputs, DEVICE memory, A = 2 for scheme 2 with polarity_split, else 1:
 *   d_w              float32 [A][T][H][W], the final state
 *   d_resistance     float32 [A][T][H][W], resistance_exp of it
 *   d_block_current  float64 [A][T][S][H / memsize][W / memsize], may be NULL (snap_every, memsize and v_ds are then not
 *                    read): the block maximum of v_ds / R after the slices at which nsof_accum_step_events(snap_every)
 *                    snapshots -- slice indices 0, k, 2k, ... -- so S = (n_slices - 1) / snap_every + 1.  No full-resolution
 *                    snapshot is kept.
 * Contract: trial t equals, bit for bit, the single-array path with trial t's planes -- nsof_accum_set_param_maps, then
 * nsof_accum_step_events, nsof_accum_read_w / _read_resistance and nsof_accum_block_current_dev of snapshot s -- the same
 * per-pixel arithmetic, neg_lam = (float)(-ln(Roff / Ron)) formed the same way, the state starting at the trial's wini.
 * Which slices drive which pixel depends on the events alone (scheme 1's per-slice count against theta, scheme 2's
 * refractory walk: one next_ok plane per array), so per group of up to 32 slices the events are scattered once, each
 * touched pixel is resolved once, and T states are replayed with T drives.  That holds with silent_v in the dead zone
 * [voff, von] of every pixel of every trial; otherwise every pixel is visited with its per-trial silent drive (a plain
 * form).  The call returns once the run has finished (it synchronises the context's stream).
 * NSOF_EINVAL, before anything is allocated, uploaded or launched: what the single-array entries refuse (geometry, scheme,
 * params, theta < 1 or theta != 1 with scheme 2, slice bounds, an event outside the sensor), n_trials < 1, a key outside
 * [0, NSOF_ACCUM_KEY_COUNT) or given twice, a NULL plane, plane_trials[j] other than 1 or n_trials, block currents with
 * snap_every < 1, memsize outside [1, min(H, W)] or v_ds <= 0, and any plane value outside the domain
 * nsof_accum_set_param_maps checks (ln(Roff / Ron) finite included) -- the message naming key, trial, row, column and value
 * of the first one, planes in the order given.  NSOF_EUNSUPPORTED (likewise): more than 65535 trials or 2^31 events ("too
 * large for one launch"). */
int nsof_accum_trials_dev(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v, float silent_v,
                          const nsof_accum_params* params, int theta, const int16_t* x, const int16_t* y, const int8_t* p,
                          const int64_t* t, const int64_t* slice_bounds, int64_t n_slices, int64_t snap_every, int memsize,
                          double v_ds, int n_trials, int n_maps, const int* keys, const float* const* planes,
                          const int* plane_trials, float* d_w, float* d_resistance, double* d_block_current);
/* Cycle-to-cycle (C2C) write noise of the trial run: the same device, driven by the same pulse, moves by a different amount
 * each time.  One standard variate xi belongs to each update, a pure function of (seed, array a, trial t, pixel = y * W + x,
 * slice = the absolute 0-based index of the slice in the call's slice_bounds); nothing is consumed, so xi does not depend on
 * the grouping, the snapshot cadence, the number of trials or which kernel form runs.
 *   generator  Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), counter =
 *              (pixel, slice & 0xffffffff, slice >> 32, t + 65536 * a), key = (seed & 0xffffffff, seed >> 32)
 *   variate    S = the sum of the 16 bytes of the four output words (0..4080); xi = (float)(S - 2040) * 0x1.bb688cp-9f, the
 *              float32 of 1 / sqrt(87380): Irwin-Hall(16) on bytes, mean 0, variance 1, support +-6.90.  Integer steps and
 *              one rounded multiply: host and device agree bit for bit
 *   update     with g = ka * pow(1 - w*s, b) as the noiseless update forms it: f = max(0, 1 + sigma * xi) -- product rounded,
 *              sum rounded, clamped at 0: a pulse may fail to switch, it never switches backwards --, wn = w + (g * f) * dt,
 *              then the clip.  sigma = sigma_off where the drive took the V < voff branch, sigma_on where it took V > von; a
 *              dead-zone drive is untouched.  The active and the silent drive alike. */
typedef struct nsof_accum_c2c {
    uint64_t seed;
    float sigma_on, sigma_off;
} nsof_accum_c2c;
/* nsof_accum_trials_dev with C2C noise: the same arguments, then c2c.  c2c == NULL, or both sigmas 0, is the noiseless run:
 * nsof_accum_trials_dev's kernels and bits (that entry IS this one called with NULL).  NSOF_EINVAL, before anything is
 * allocated: a sigma that is negative or not finite, the message naming the field and the value. */
int nsof_accum_trials_c2c_dev(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split, float active_v,
                              float silent_v, const nsof_accum_params* params, int theta, const int16_t* x, const int16_t* y,
                              const int8_t* p, const int64_t* t, const int64_t* slice_bounds, int64_t n_slices,
                              int64_t snap_every, int memsize, double v_ds, int n_trials, int n_maps, const int* keys,
                              const float* const* planes, const int* plane_trials, float* d_w, float* d_resistance,
                              double* d_block_current, const nsof_accum_c2c* c2c);
/* The variates of that run on the HOST (no context, no device): out[i] = xi of (seed, array, trial, pixel, slice + i) for
 * i in [0, n_slices).  For the frame-driven run below: array = 0, pixel = the cell, slice = the pair index. */
void nsof_accum_c2c_noise(uint64_t seed, int array, int trial, uint32_t pixel, int64_t slice, int64_t n_slices, float* out);
/* The trial run as an OBJECT: the T states, the per-array refractory maps and the slice counter stay in HBM and the stream is
 * handed over chunk by chunk -- nsof_accum_trials_dev without its limit on the length of a recording, with read-outs between
 * chunks and with a drive voltage per trial.  A run cut into chunks at ANY slices equals the one-shot run bit for bit: the
 * groups are cut and the snapshots timed by the object's absolute slice counter, scheme 2's next_ok carries over, and a
 * noise variate is a function of the absolute slice index.  (nsof_accum_trials_dev / _c2c_dev are create, one step, the
 * read-outs and destroy over this implementation.)
 * nsof_accum_trials_create: geometry, scheme, polarity_split, params, theta, n_trials, the plane list and c2c exactly as
 * nsof_accum_trials_c2c_dev takes them (c2c may be NULL).  active_v [n_active] and silent_v [n_silent] are HOST arrays, each
 * of 1 value (all trials) or n_trials values (trial t drives with active_v[t], leaks with silent_v[t]; scheme 2's active
 * drive is the float32 sum silent_v[t] + active_v[t]).  With a voltage per trial every trial has its own drive planes, and
 * the touched-pixels form runs only if silent_v[t] lies in the dead zone of every pixel of trial t for EVERY t -- one leaking
 * trial puts all trials on the every-pixel form (same bits, trial by trial).  theta stays one value.  snap_every, memsize and
 * v_ds are fixed for the object's life; memsize == 0: no block currents (snap_every and v_ds are then not read).
 * NSOF_EINVAL / NSOF_EUNSUPPORTED before anything is allocated, uploaded or launched: everything nsof_accum_trials_c2c_dev
 * refuses that does not concern the stream, n_active / n_silent other than 1 or n_trials (or a NULL array), and a voltage
 * that is not finite, the message naming the trial. */
typedef struct nsof_accum_trials nsof_accum_trials;
int nsof_accum_trials_create(nsof_ctx* ctx, int height, int width, int scheme, int polarity_split,
                             const nsof_accum_params* params, int theta, int n_trials, int n_maps, const int* keys,
                             const float* const* planes, const int* plane_trials, const nsof_accum_c2c* c2c,
                             const float* active_v, int n_active, const float* silent_v, int n_silent, int64_t snap_every,
                             int memsize, double v_ds, nsof_accum_trials** out);
void nsof_accum_trials_destroy(nsof_accum_trials* a);
/* The snapshot slices -- absolute indices 0, k, 2k, ... -- among the n_slices slices from `counter` on (pure host arithmetic),
 * and the same for the object's own counter and cadence (0 without block currents): S_chunk of the next step. */
int64_t nsof_accum_snaps_between(int64_t counter, int64_t n_slices, int64_t snap_every);
int64_t nsof_accum_trials_snaps_in(const nsof_accum_trials* a, int64_t n_slices);
/* Advance over n_slices slices of HOST event arrays (as nsof_accum_step_events takes them; only this chunk is staged, and
 * the arrays are not retained: the call returns once the chunk has run).  d_block_current (DEVICE, may be NULL where
 * S_chunk = nsof_accum_trials_snaps_in(a, n_slices) is 0) receives float64 [A][T][S_chunk][rows][cols], the block maxima after
 * the snapshot slices inside the chunk; *n_snaps (may be NULL) = S_chunk.  n_slices == 0 does nothing.  A refused step --
 * NSOF_EINVAL for bad bounds, a NULL array or an event outside the sensor, NSOF_EUNSUPPORTED for 2^31 events or more in ONE
 * step -- launches nothing and leaves the object as it was. */
int nsof_accum_trials_step(nsof_accum_trials* a, const int16_t* x, const int16_t* y, const int8_t* p, const int64_t* t,
                           const int64_t* slice_bounds, int64_t n_slices, double* d_block_current, int64_t* n_snaps);
/* The same step over a chunk of a DEVICE stream: the four arrays, n_events and the host bounds as
 * nsof_accum_set_events_dev takes them, checked and staged by the same code (one check, one staging, one message for both
 * kinds of accumulator); everything else as nsof_accum_trials_step, the 2^31-event limit of ONE step included.  States,
 * block currents and surfaces equal the host entry's bit for bit.  Waits for the context's stream twice: for the verdict,
 * and when the chunk has run. */
int nsof_accum_trials_step_dev(nsof_accum_trials* a, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                               int64_t n_events, const int64_t* slice_bounds, int64_t n_slices, double* d_block_current,
                               int64_t* n_snaps);
/* Read-outs to DEVICE memory, asynchronous on the context's stream: the states and their resistances, float32 [A][T][H][W];
 * the block maxima of v_ds / R of the CURRENT states, float64 [A][T][rows][cols] (needs memsize). */
int nsof_accum_trials_w_dev(nsof_accum_trials* a, float* d_out);
int nsof_accum_trials_resistance_dev(nsof_accum_trials* a, float* d_out);
int nsof_accum_trials_block_current_dev(nsof_accum_trials* a, double* d_out);
/* The surface of array `which` of every trial as frames [T][H][W] (mode as nsof_accum_surface_u8_dev: 0 current, 1 state):
 * trial t's frame starts trial_stride after trial t-1's, its rows are row_stride apart (u8: both in bytes = pixels, row_stride
 * >= W; f32: both in BYTES, multiples of 4, row_stride >= 4 * W; trial_stride >= H * row_stride).  Frame t holds, bit for bit,
 * what nsof_accum_surface_u8_dev / _f32_dev write for an accumulator with trial t's planes in the same state.  One launch;
 * asynchronous on the context's stream. */
int nsof_accum_trials_surface_u8_dev(nsof_accum_trials* a, int which, int mode, uint8_t* d_out, ptrdiff_t row_stride,
                                     ptrdiff_t trial_stride);
int nsof_accum_trials_surface_f32_dev(nsof_accum_trials* a, int which, int mode, float* d_out, ptrdiff_t row_stride_bytes,
                                      ptrdiff_t trial_stride_bytes);
/* Checkpoint / resume through the HOST: w float32 [A][T][H][W], next_ok int64 [A][H][W] (one plane per array, as the kernels
 * hold it; zeros for scheme 1) and the slice counter.  Any output of read_state may be NULL.  write_state: n_w_planes must be
 * A * T and, where next_ok_in is given, n_next_ok_planes A (NSOF_EINVAL otherwise, nothing written); next_ok_in == NULL writes
 * zeros (n_next_ok_planes is not read).  Both synchronise.  reset: back to the wini planes, next_ok zero, counter 0. */
int nsof_accum_trials_read_state(nsof_accum_trials* a, float* w_out, int64_t* next_ok_out, int64_t* slice_counter);
int nsof_accum_trials_write_state(nsof_accum_trials* a, const float* w_in, int64_t n_w_planes, const int64_t* next_ok_in,
                                  int64_t n_next_ok_planes, int64_t slice_counter);
int nsof_accum_trials_reset(nsof_accum_trials* a);
/* C2C write noise in the FRAME-driven run, and a pair-index origin: nsof_accum_frames_f64_maps_dev's arguments, then c2c and
 * first_pair.  The same generator and the same nsof_accum_c2c as the event path.  For trial t, cell i = r * W + c of the
 * compressed grid as passed, and frame pair q = first_pair + f (f = 0 .. n_frames - 2):
 *   V       the pair's drive voltage exactly as the noiseless run forms it
 *   branch  decided against that cell's own voff / von: V < voff uses sigma_off, V > von uses sigma_on, anything else is the
 *           dead zone: no noise and no draw
 *   xi      nsof_accum_c2c_noise(seed, array = 0, trial = t, pixel = i, slice = q): the counter (i, q & 0xffffffff, q >> 32,
 *           t), the key (seed & 0xffffffff, seed >> 32).  The frame path is "array 0"; its "slice" is the pair index
 *   factor  f = max(0, u) with u = 1.0 + (double)sigma * (double)xi: sigma is the float of nsof_accum_c2c, its product with
 *           the float32 xi is exact in double, the sum is rounded once.  A pulse may fail to switch, it never switches
 *           backwards
 *   update  ONE factor per pair, held for all n_sub_steps sub-steps of that pair: every sub-step is nw = w + (dwdt * f) *
 *           dts, then the clip to [0, 1], each operation rounded on its own.  A "cycle" is one write, one frame interval;
 *           the sub-steps are the Euler integration of that one pulse, so the result does not depend on n_sub_steps as a
 *           noise setting
 * sigma == 0 for the branch taken gives the noiseless bits for that pair.  c2c == NULL, or both spreads 0, is the noiseless
 * run: the kernels nsof_accum_frames_f64_maps_dev launched before this entry existed are launched (that entry IS this one
 * called with NULL, 0), and first_pair has no effect.  The result is a pure function of (seed, t, i, q) and the inputs: it
 * does not depend on how many trials run, on the source of the device model, or on how a video is cut into calls -- frames
 * [0, k] and then frames [k, n) with wini = the state after the first call (a plane) and first_pair = k give the one-shot
 * run's w, res and current bit for bit.
 * NSOF_EINVAL, before anything is uploaded, launched or written: a sigma that is negative or not finite (the message names
 * the field and the value), first_pair < 0 or first_pair + n_frames beyond int64.  NSOF_EUNSUPPORTED (likewise): noise with
 * n_trials > 65535, since the trial shares the counter word's layout with the event path.  Then everything
 * nsof_accum_frames_f64_maps_dev refuses. */
int nsof_accum_frames_f64_c2c_dev(nsof_ctx* ctx, const double* d_imgs, int n_frames, int height, int width, double dt,
                                  int n_sub_steps, double th1, double th2, double v_ds, const nsof_accum_params* params,
                                  int n_trials, int n_maps, const int* keys, const double* const* planes,
                                  const int* plane_trials, double* d_w, double* d_res, double* d_current,
                                  const nsof_accum_c2c* c2c, int64_t first_pair);
/* The host twin (nsof_accum_frames_f64_maps with c2c and first_pair): the one host path -- validate, upload, the device
 * entry, download, synchronise.  The device entry's bits. */
int nsof_accum_frames_f64_c2c(nsof_ctx* ctx, const double* imgs, int n_frames, int height, int width, double dt,
                              int n_sub_steps, double th1, double th2, const nsof_accum_params* params, int n_trials,
                              int n_maps, const int* keys, const double* const* planes, const int* plane_trials,
                              double* w_out, double* res_out, const nsof_accum_c2c* c2c, int64_t first_pair);
/* compress_image of the same script (:111-121) for a stack of 8-bit DEVICE frames: imresize(im2double(frame), [out_h
 * out_w], 'lanczos3') of n_frames frames into d_out [n_frames][out_h][out_w] (DEVICE, dense float64).  d_frames points
 * at the first pixel of the region to compress -- a crop is a pointer offset plus width and height -- with row_stride and
 * frame_stride in bytes under the layout rule above.  wts_y / ind_y [out_h][taps_y] and wts_x / ind_x [out_w][taps_x] are
 * HOST tables: per output sample its tap weights and the mirrored 0-based source indices of the taps
 * (nsof_lanczos3_contributions, or the Python mirror's nsof.frames._contributions); they are copied through the
 * context's table buffer and not retained.  Arithmetic, order included: im2double(v) = double(v) / 255.0; the axis with
 * the smaller scale goes first (out_h * width <= out_w * height: rows first); every output starts at 0.0 and takes its
 * taps left to right, acc = acc + w[k] * v[k], the product rounded before the sum; the intermediate is float64.  With the
 * mirror's tables the result equals the mirror's bit for bit.  Needs 1 <= out_w <= width and 1 <= out_h <= height: a scale
 * above 1 is NSOF_EUNSUPPORTED; a null pointer, n_frames < 1, a tap count < 1, an empty output, a row stride below the
 * width or a source index outside the frame NSOF_EINVAL -- all before anything is launched.  Asynchronous on the
 * context's stream (it waits only for its own previous table upload, or to grow a buffer). */
int nsof_frames_compress_u8_dev(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames, ptrdiff_t row_stride,
                                ptrdiff_t frame_stride, int width, int height, int out_w, int out_h, const double* wts_y,
                                const int32_t* ind_y, int taps_y, const double* wts_x, const int32_t* ind_x, int taps_x,
                                double* d_out);
/* The tap table of one axis of that resize, host only (the `contributions` routine of imresize.m as nsof.frames states
 * it): *taps = the taps per output sample (the columns that carry a non-zero weight for some output); with wts != NULL
 * also wts / ind [out_len][*taps] (cap_taps >= *taps, else NSOF_EINVAL), indices mirrored at both image ends as often as
 * a window wider than the image needs.  With wts == NULL only the count. */
int nsof_lanczos3_contributions(int in_len, int out_len, double* wts, int32_t* ind, int cap_taps, int* taps);
/* slice_indices() of event_mem_sim.py:78-83 on a HOST timestamp array: returns the number
 * of bounds and fills idx (if not NULL) with up to cap entries. */
int64_t nsof_accum_slice_bounds(const int64_t* t, int64_t n, int64_t slice_us, int64_t* idx, int64_t cap);
/* slice_indices() on a DEVICE timestamp array: nsof_accum_slice_bounds' result, idx a HOST array (up to cap entries, cap
 * < 2^31; a pinned table of cap entries carries them).  One pass checks the order and reads t[0] and t[n - 1]; with idx,
 * one thread per bound then searches the sorted array for the first index with t >= t[0] + i * slice_us -- on a sorted
 * array exactly the host scan's result.  Returns the number of bounds, or a negative status: NSOF_EINVAL for t not
 * non-decreasing (the message names the first e with t[e] < t[e-1]).  Works on the context's stream and waits for it
 * ONCE per call: the verdict, the two times and the table come back in one copy.  |t| < 2^62. */
int64_t nsof_accum_slice_bounds_dev(nsof_ctx* ctx, const int64_t* d_t, int64_t n, int64_t slice_us, int64_t* idx, int64_t cap);

/* ---- ROI gating: the rectangles the gated path crops -------------------------------------------- */
/* opticalFlow3D's gating arithmetic (optical_flow_seg.py:211-252 with :115-121, :426-435) for ONE gating slice, pure
 * host code (maps are at most 24 x 13 cells): current [rows][cols] (device currents in ampere, the constructed3DMatrix
 * slice) -> gray = uint8(clip(-3366/log10(I) - 306, 0, 255)) -> cells with gray >= thres inside the
 * (frame_h / memsize) x (frame_w / memsize) transition picture -> connected components (connectivity 4 or 8, labelled
 * in raster order of their first cell) -> per component (flag 1) or for the union box (flag 2) the rectangle
 * x0 = max(x*memsize - extend_left, 0), y0 = max(y*memsize - extend_upper, 0), x1 = min((x+a)*memsize + extend_right,
 * frame_w), y1 = min((y+b)*memsize + extend_lower, frame_h).  rects receives up to max_rects rows of (x0, y0, x1, y1);
 * returns the number of rectangles (which may exceed max_rects: call again with more room), 0 when nothing crosses
 * the threshold, or a negative nsof_status. */
int nsof_roi_from_surface(const double* current, int rows, int cols, int frame_w, int frame_h, int memsize, int thres,
                          int extend_left, int extend_right, int extend_upper, int extend_lower, int connectivity,
                          int flag, int* rects, int max_rects);

/* Device twin of nsof_roi_from_surface (replaces optical_flow_seg.py:115-121,211-252 for maps that are already in HBM):
 * n_maps gating maps at once -- d_current: device currents, double, map k at d_current + k*map_stride (rows x cols
 * cells, any size up to 2^27 cells; NSOF_ESHAPE when the map is larger than the frame's transition picture); gray map,
 * threshold, connected components in raster order, rectangles as above.  Maps of at most 64 x 64 cells take one
 * wavefront each (bit-parallel flood fill); larger maps a union-find over the context's workspace, processed in chunks
 * of maps when a batch's scratch is large.  d_counts[k] = number of rectangles of map k (may exceed max_rects; only the first max_rects
 * are stored), d_rects[k][max_rects][4] = (x0, y0, x1, y1); d_gray (optional, may be NULL): the 8-bit gating maps
 * [n_maps][rows][cols].  All DEVICE memory; asynchronous on the context's stream. */
int nsof_roi_from_surface_dev(nsof_ctx* ctx, const double* d_current, int n_maps, size_t map_stride, int rows, int cols,
                              int frame_w, int frame_h, int memsize, int thres, int extend_left, int extend_right,
                              int extend_upper, int extend_lower, int connectivity, int flag, int max_rects, int* d_counts,
                              int* d_rects, unsigned char* d_gray);
/* Gate statistics of a variability study (the stacks nsof_accum_frames_f64_maps_dev writes): d_current [n_trials][n_frames]
 * [rows][cols] are the device currents of the trials, d_nominal [n_frames][rows][cols] those of the nominal array.  A cell
 * is gated when its gating value -- the 8-bit value nsof_roi_from_surface_dev forms, the bytes of its d_gray -- is >= thres.
 * d_counts int32 [n_frames][rows][cols]: the number of trials in which the cell is gated (gate probability = count /
 * n_trials); d_flips int32 [n_trials][n_frames]: the number of cells of that trial's map whose gated bit differs from the
 * nominal's.  Integer sums without atomics: exact, whatever the order.  One launch, any n_trials, maps from one cell on;
 * all DEVICE memory, asynchronous on the context's stream.  NSOF_EUNSUPPORTED: a map above 2^27 cells, or sizes beyond one
 * launch. */
int nsof_gate_stats_dev(nsof_ctx* ctx, const double* d_current, const double* d_nominal, int n_trials, int n_frames, int rows,
                        int cols, int thres, int* d_counts, int* d_flips);

/* ---- next: motion-segmentation head on the flow field --------------------- */
/* Replaces, in /root/reference/optical_flow_seg.py, the chain
 *   mag, ang = cv2.cartToPolar(flow_x, flow_y)                         :283, :503
 *   motion_mask[mag > SEG_TH] = 255                                     :346-347
 *   kernel = cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (10, 10))     :350
 *   5 x { cv2.dilate(mask, kernel); cv2.erode(mask, kernel) }           :351-353
 *   cv2.threshold(mask, 1, 255, cv2.THRESH_BINARY)                      :356
 * (process_flow_region :322-357; baseline copy :503-537).  Both operations take
 * dst(x,y) = max|min over element(i,j) != 0 of src(x + j - ax, y + i - ay), anchor = ksize/2,
 * pixels outside the image do not take part (cv2's default morphology border). */
enum { NSOF_MORPH_RECT = 0, NSOF_MORPH_CROSS = 1, NSOF_MORPH_ELLIPSE = 2 };   /* cv2.MORPH_RECT/CROSS/ELLIPSE */
enum { NSOF_MORPH_ERODE = 0, NSOF_MORPH_DILATE = 1 };
/* cv2.getStructuringElement(shape, (kw, kh)) -> out[kh][kw] of 0/1 (HOST). */
int nsof_structuring_element(int shape, int kw, int kh, uint8_t* out);
/* cv2.dilate / cv2.erode for two-valued masks on DEVICE memory: non-zero source pixels count as set, the
 * result is 0/255.  elem = HOST [kh][kw] (non-zero = member), up to 32x32 with at most 8 distinct rows;
 * anchor (-1,-1) = centre; `iterations` repeats the operation.  strides in bytes. */
int nsof_morph_binary_u8_dev(nsof_ctx* ctx, int op, const uint8_t* d_src, ptrdiff_t src_stride, int width,
                             int height, const uint8_t* elem, int kw, int kh, int anchor_x, int anchor_y,
                             int iterations, uint8_t* d_dst, ptrdiff_t dst_stride);
/* The whole head on a DEVICE flow field [h][w][2] float32 (row stride in floats, even): mask = 255 where
 * sqrt(u^2 + v^2) (in double, as cartToPolar sees the float64 canvas) > thresh, then `iterations` x
 * (dilate, erode) with the ksize x ksize ellipse, all in one pass over the flow plus one fused launch on the
 * bit-packed mask.  d_mask [h][mask_stride] uint8. */
int nsof_motion_mask_dev(nsof_ctx* ctx, const float* d_flow, ptrdiff_t flow_stride_floats, int width, int height,
                         double thresh, int ksize, int iterations, uint8_t* d_mask, ptrdiff_t mask_stride);
/* The head over the boxes of a whole sequence (optical_flow_seg.py task_results :253-320, the full-frame baseline
 * :503-537).  d_flows: float32 [n_pairs][height][width][2] (dense, 8-byte aligned); d_masks: uint8
 * [n_pairs][height][width] (dense).  box_counts[n_pairs] and boxes[sum of counts][4] of (x0, y0, x1, y1) are HOST
 * arrays: a pair's boxes are consecutive and in paste order; box_counts == NULL is one whole-frame box per pair.
 * Every pixel of every canvas is written: the mask of the LAST box that covers it, computed as nsof_motion_mask_dev
 * computes it on the crop flow[y0:y1, x0:x1] (the crop's edges are image borders), or 0 where no box covers it.
 * Empty boxes (x1 <= x0 or y1 <= y0) are skipped.  Boxes leaving the frame, n_pairs outside 1..65535, ksize outside
 * 1..32, iterations outside 0..16 and null pointers return an nsof_status before anything is launched.
 * Asynchronous: the box and job tables go up through a pinned copy that a later call rewrites only after this
 * upload has finished (waiting for that, or growing the tables or the workspace, are its only waits). */
int nsof_motion_mask_sequence_dev(nsof_ctx* ctx, int n_pairs, const float* d_flows, int width, int height,
                                  const int32_t* box_counts, const int32_t* boxes, double thresh, int ksize,
                                  int iterations, uint8_t* d_masks);
/* optical_flow_seg.py calculate_pixel_accuracy of n masks against ground-truth frames, into the DEVICE doubles
 * d_out[n]: d_masks uint8 [n][height][width] (dense, 0/255), d_gt interleaved BGR uint8 frames (strides in bytes),
 * binarised as (BGR2GRAY(gt) > 127) ? 255 : 0 with cv2's fixed-point weights.  d_out[i] = (double)equal_pixels /
 * (double)(width * height) * 100.0; the pixels are counted in integers, so the result is exact.  Asynchronous. */
int nsof_pixel_accuracy_u8_batch_dev(nsof_ctx* ctx, int n, const uint8_t* d_masks, const uint8_t* d_gt,
                                     ptrdiff_t gt_row_stride, ptrdiff_t gt_frame_stride, int width, int height,
                                     double* d_out);
/* Same with HOST pointers (flow row stride in bytes: ROI views of the flow canvas are passed as they are). */
int nsof_motion_mask(nsof_ctx* ctx, const float* flow, ptrdiff_t flow_stride_bytes, int width, int height,
                     double thresh, int ksize, int iterations, uint8_t* mask, ptrdiff_t mask_stride);

/* ---- next: frame prediction by flow warp + SSIM --------------------------- */
/* Replaces, in /root/reference/optical_flow_prediction.py,
 *   flow_map = (grid + flow).astype(np.float32)                                         :289-290, :338-339, :581-582
 *   cv2.remap(next_frame[:,:,c], flow_map[...,0], flow_map[...,1], cv2.INTER_LINEAR,
 *             borderMode=cv2.BORDER_REPLICATE)      (gated path)                        :293-300, :342-349
 *   cv2.remap(next_frame[:,:,c], map_x, map_y, cv2.INTER_LINEAR)   (baseline, constant 0) :584-586
 *   structural_similarity(true[:,:,2], prediction[:,:,2], data_range=255.0)             :113-115
 * remap follows cv2's 8-bit fixed point: map rounded to 1/32 px (half to even), integer part saturated to int16,
 * 15-bit weights, (sum + 2^14) >> 15. */
enum { NSOF_BORDER_CONSTANT = 0, NSOF_BORDER_REPLICATE = 1 };   /* cv2.BORDER_CONSTANT / cv2.BORDER_REPLICATE */
/* 8-bit luma of an interleaved 3-channel DEVICE frame as cv2.cvtColor computes it (fixed point, (sum + 2^14) >> 15):
 * bgr_weights = 0 -> COLOR_RGB2GRAY weights in memory order (what the scripts apply to imread's B,G,R frames,
 * optical_flow_seg.py:442-443), 1 -> COLOR_BGR2GRAY (:447).  Strides in bytes.  Lets decoded frames stay in HBM up
 * to the flow call. */
int nsof_gray_u8_dev(nsof_ctx* ctx, const uint8_t* d_src, ptrdiff_t src_stride, int width, int height, int bgr_weights,
                     uint8_t* d_dst, ptrdiff_t dst_stride);
/* cv2.remap for uint8 sources with 1 or 3 interleaved channels and two float32 maps, all on the DEVICE.
 * Strides of the images in bytes, of the maps in floats.  Source up to 32767 x 32767. */
int nsof_remap_linear_u8_dev(nsof_ctx* ctx, const uint8_t* d_src, ptrdiff_t src_stride, int src_w, int src_h,
                             int channels, const float* d_map_x, ptrdiff_t map_x_stride_floats,
                             const float* d_map_y, ptrdiff_t map_y_stride_floats, int dst_w, int dst_h,
                             int border_mode, int border_value, uint8_t* d_dst, ptrdiff_t dst_stride);
/* The prediction step for the region [y0,y1) x [x0,x1) of a frame, fused: map = float32(float64(grid) + sign *
 * float64(flow)) is formed in the kernel from the DEVICE flow canvas [height][flow_stride_floats] (u,v) and the
 * region of d_out (a frame-sized image; the caller pre-fills it with the frame, prediction.py:263) is overwritten
 * with the warped d_frame.  sign = -1 for Farneback flow (prediction.py:545). */
int nsof_predict_warp_u8_dev(nsof_ctx* ctx, const uint8_t* d_frame, ptrdiff_t frame_stride, int width, int height,
                             int channels, const float* d_flow, ptrdiff_t flow_stride_floats, int sign,
                             int x0, int y0, int x1, int y1, int border_mode, uint8_t* d_out, ptrdiff_t out_stride);
/* Same with HOST pointers; flow_crop points at the region's first flow vector (row stride in bytes), i.e. the view
 * flow[y0:y1, x0:x1] of a float32 canvas.  Only the region of `out` is written. */
int nsof_predict_warp_u8(nsof_ctx* ctx, const uint8_t* frame, ptrdiff_t frame_stride, int width, int height,
                         int channels, const float* flow_crop, ptrdiff_t flow_stride_bytes, int sign,
                         int x0, int y0, int x1, int y1, int border_mode, uint8_t* out, ptrdiff_t out_stride);
/* skimage.metrics.structural_similarity(a, b, data_range=...) with its defaults (7x7 uniform window, sample
 * covariance, K1 0.01, K2 0.03) for 8-bit images on the DEVICE; pixel_step selects one channel of an interleaved
 * image (3 for true[:,:,2] with the pointer advanced by 2).  *ssim_out is a HOST double; synchronises. */
int nsof_ssim_u8_dev(nsof_ctx* ctx, const uint8_t* d_a, ptrdiff_t a_stride, int a_pixel_step, const uint8_t* d_b,
                     ptrdiff_t b_stride, int b_pixel_step, int width, int height, double data_range,
                     double* ssim_out);
int nsof_ssim_u8(nsof_ctx* ctx, const uint8_t* a, ptrdiff_t a_stride, int a_pixel_step, const uint8_t* b,
                 ptrdiff_t b_stride, int b_pixel_step, int width, int height, double data_range, double* ssim_out);
/* The prediction step of every pair of a sequence in ONE launch (optical_flow_prediction.py:435-681, task_results
 * :257-361 and the full-frame baseline :569-591).  d_frames: n_pairs + 1 interleaved 3-channel (BGR) uint8 frames,
 * strides in bytes; pair k reads frame k + 1 and the flow canvas k of d_flows, float32 [n_pairs][height][width][2] (dense,
 * 8-byte aligned), and writes prediction k of d_out, uint8 [n_pairs][height][width][3] (dense) -- in full: pixels
 * outside the pair's region are copies of frame k + 1, so d_out needs no pre-fill.  Region: with d_counts / d_rects
 * (the device table of nsof_roi_from_surface_dev, [n_maps] and [n_maps][max_rects][4], the table the ROI flow call
 * consumed) the rectangles of map k + gate_frame (gate_frame 0 or 1, as nsof_farneback_u8_roi_sequence_dev), their union
 * for merge_padding < 0 (FLAG 1 with MERGE_FLAG False; FLAG 2, one box), their bounding box padded by merge_padding
 * and clipped to the frame for merge_padding >= 0 (MERGE_FLAG True, PADDING 20); a map without rectangles leaves the
 * frame as it is.  The caller guarantees counts <= max_rects (the launch cannot see them beforehand; larger counts are
 * read as max_rects).  d_counts == NULL: the whole frame (the baseline; border_mode NSOF_BORDER_CONSTANT, value 0).
 * Every pixel is computed as nsof_predict_warp_u8_dev computes it (map = float32(float64(grid) + sign * flow)), so
 * prediction k equals that entry applied box by box onto a copy of the frame, bit for bit.  Asynchronous. */
int nsof_predict_sequence_u8_dev(nsof_ctx* ctx, int n_pairs, const uint8_t* d_frames, ptrdiff_t row_stride,
                                 ptrdiff_t frame_stride, int width, int height, const float* d_flows, int sign,
                                 const int32_t* d_counts, const int32_t* d_rects, int n_maps, int max_rects,
                                 int gate_frame, int merge_padding, int border_mode, uint8_t* d_out);
/* nsof_ssim_u8_dev of n image pairs (pair i at d_a + i * a_item_stride, d_b + i * b_item_stride, bytes) into the DEVICE
 * doubles d_out[n]: same tile grid and reduction order per pair, so d_out[i] == nsof_ssim_u8_dev of pair i exactly.
 * Asynchronous: never waits for the stream (only growing the context's workspace, on a first or larger call, does). */
int nsof_ssim_u8_batch_dev(nsof_ctx* ctx, int n, const uint8_t* d_a, ptrdiff_t a_stride, ptrdiff_t a_item_stride,
                           int a_pixel_step, const uint8_t* d_b, ptrdiff_t b_stride, ptrdiff_t b_item_stride,
                           int b_pixel_step, int width, int height, double data_range, double* d_out);
/* Middlebury colour coding (flow_viz.flow_to_image, optical_flow_prediction.py:12-19, :524, :578) of n float32 (u,v)
 * flow fields on the DEVICE: item i at d_flows + i*item_stride_floats, rows row_stride_floats apart; flow := sign*flow
 * (sign +1 / -1), then np.clip(flow, 0, clip_flow) when clip_flow >= 0, then normalised by the item's own max
 * magnitude + 1e-5 (max_flow < 0) or by max_flow + 1e-5.  d_out uint8 [H][W][3] per item (strides in bytes), RGB, or
 * BGR with convert_to_bgr.  d_norms (optional, DEVICE float32 [n]) receives the float32 divisor used per item.
 * Asynchronous on the context's stream; flows must be finite. */
int nsof_flow_to_image_dev(nsof_ctx* ctx, int n, const float* d_flows, ptrdiff_t row_stride_floats,
                           ptrdiff_t item_stride_floats, int width, int height, int sign, double clip_flow,
                           double max_flow, int convert_to_bgr, uint8_t* d_out, ptrdiff_t out_row_stride,
                           ptrdiff_t out_item_stride, float* d_norms);
/* Statistics of an ensemble of flow fields against a reference flow (csrc/flow_ensemble.hip): the
 * reduction of the Monte-Carlo trials' flows of a study.  Field f of trial t is an interleaved (u, v) float32 image at
 * d_flows + t*trial_stride_floats + f*field_stride_floats, rows row_stride_floats apart (even, the base 8-byte aligned);
 * d_ref: n_fields such fields with strides of their own, or NULL for a zero reference.  Per pixel, for the trials in
 * index order, in double, every operation rounded on its own:
 *     du = (double)flow.u - (double)ref.u, dv likewise;  sum += (du, dv);  sq += (du*du, dv*dv, du*dv);
 *     e2 = du*du + dv*dv;  if (e2 > m) m = e2     (a NaN never enters the maximum, +inf does)
 * into d_sum [n_fields][H][W][2], d_sq [n_fields][H][W][3] and d_epe2_max [n_fields][H][W].  accumulate 0 starts them from
 * zero (they are written, not read), 1 continues from the stored values: a run cut into chunks of trials at any points
 * equals the one-shot run bit for bit.  Per (trial, field), [n_trials][n_fields]: d_outliers counts the pixels with
 * e2 > tau*tau (formed once on the host), d_nonfinite those with !(e2 < inf), d_aee = (sum over the pixels of sqrt(e2)) /
 * (W*H) with IEEE propagation of non-finite pixels; the pixel sum has a fixed order that depends on the image size alone
 * (per wave, per workgroup, then the workgroups' partials in index order; no float atomics), so d_aee has the same bits
 * from run to run and however the trials are chunked.  All pointers DEVICE memory; asynchronous on the context's stream
 * (only growing the context's workspace, on a first or larger call, waits for it).
 * NSOF_EINVAL, nothing launched and no output touched, the value named in nsof_last_error: n_trials, n_fields, width or
 * height < 1, a null pointer other than d_ref, an odd or too-short row stride or a base or stride that is not 8-byte
 * aligned, accumulate outside {0, 1}, tau negative or NaN.  NSOF_EUNSUPPORTED (likewise): W*H > 2^27, or sizes beyond
 * one launch (height > 262140, more than 65535 fields). */
int nsof_flow_ensemble_dev(nsof_ctx* ctx, int n_trials, int n_fields, const float* d_flows, ptrdiff_t row_stride_floats,
                           ptrdiff_t field_stride_floats, ptrdiff_t trial_stride_floats, int width, int height,
                           const float* d_ref, ptrdiff_t ref_row_stride_floats, ptrdiff_t ref_field_stride_floats,
                           double tau, int accumulate, double* d_sum, double* d_sq, double* d_epe2_max, double* d_aee,
                           int32_t* d_outliers, int32_t* d_nonfinite);

/* Event streams from frame sequences (csrc/events_from_frames.hip): a per-pixel level-crossing
 * event generator, the contrast-threshold model of an event camera, in integers throughout.  d_frames: n uint8 frames
 * [height][width] in DEVICE memory, row_stride / frame_stride bytes apart (any values that keep the frames readable);
 * times: HOST int64 [n], microseconds, strictly increasing by less than 2^31; lut: HOST int32 [256], entries in [0, 2^30], the
 * level of a grey value (256 * i: linear, in 1/256 grey levels); L[k] = lut[F[k]].  Thresholds c_on, c_off >= 1 in the
 * table's units, or d_thr_plane != NULL: DEVICE int32 [height][width][2] (c_on, c_off) per pixel, the scalars unused.
 * Every pixel keeps a reference level r (ref_mode NSOF_EVENTS_REF_ZERO: 0; _FIRST: L[0], so that frame 0 emits nothing;
 * _GIVEN: d_ref_in, DEVICE int32 [height][width], the d_ref_out of a previous call; d_ref_in is NULL in the other modes)
 * and takes one step per frame, in order, to the level b = L[k]:
 *     b - r >= c_on:   m = (b - r) / c_on ON events at the levels r + j * c_on, j = 1..m;   r += m * c_on
 *     r - b >= c_off:  m = (r - b) / c_off OFF events at the levels r - j * c_off;          r -= m * c_off
 * after which -c_off < L[k] - r < c_on.  The events of frame 0 are stamped times[0]; those of frame k >= 1 times[k]
 * (timestamps_mode NSOF_EVENTS_T_FRAME) or, the intensity taken to move linearly from a = L[k-1] to b (_T_LINEAR),
 * times[k-1] + (|level - a| * (times[k] - times[k-1])) / |b - a| in int64, rounded down.  The stream has the frames in
 * index order and within a frame ascends by (t, ON before OFF, y, x, j): the events of frame k are
 * [frame_bounds[k], frame_bounds[k+1]), t never decreases, and with _T_FRAME and a binary sequence the order is that of
 * generate_synthetic_events (event_mem_sim.py:109-158).  A run over frames [0, n) equals one over [0, k] followed by one
 * over [k, n) from the first one's d_ref_out, bit for bit, and two runs give the same bits.
 *
 * The output size depends on the data, so there are two entries.  nsof_events_from_frames_count_dev forms the counts,
 * synchronises and fills the HOST frame_bounds_out [n + 1] (frame_bounds_out[n]: the total); nothing else is written.
 * nsof_events_from_frames_emit_dev takes those bounds back (frame_bounds, HOST [n + 1], with the arguments of the count
 * call), forms the counts again on the stream and writes frame_bounds[n] events to d_x, d_y (int16), d_p (int8: p_on or
 * p_off) and d_t (int64), DEVICE arrays of `capacity` elements, and the final r to d_ref_out (DEVICE int32
 * [height][width], may be d_ref_in, may be NULL); it is asynchronous on the context's stream (only growing the
 * context's workspace, on a first or larger call, waits for it).  The emit pass compares the total it has formed itself
 * with frame_bounds[n] on the device and writes nothing at all, d_ref_out included, if they differ: bounds of another
 * call cannot send a store past `capacity`.
 * NSOF_EINVAL, nothing launched and nothing written, the value named in nsof_last_error: n < 1, height or width < 1 or
 * above 32767, a null frames / times / lut / bounds pointer, times that do not increase strictly or a gap >= 2^31, a
 * table entry outside [0, 2^30], a scalar threshold < 1, ref_mode and d_ref_in that do not match; emit alone: an unknown
 * timestamps_mode, p_on or p_off outside an int8, capacity < frame_bounds[n], a null output array with events to write.
 * A threshold plane that holds a value < 1 is seen by the count pass only (such a pixel emits nothing): the count entry
 * returns NSOF_EINVAL without filling frame_bounds_out, the emit entry writes nothing.  NSOF_EUNSUPPORTED: a stream of
 * 2^31 or more events (the count entry, frame_bounds_out untouched: the counts are 64-bit, the total is known before
 * anything is emitted), more than 2^24 frames.
 * Workspace: both entries keep the count table in the context's workspace, 16 bytes per frame and per 256 pixels
 * (2 * n * ceil(height * width / 256) uint64: 130 KB per 1080p frame, 130 MB per 1000 of them), and the emit entry with
 * _T_LINEAR adds 24 bytes per event plus the sort's temporary storage (a few MB).  The workspace grows on demand, is
 * never shrunk before nsof_destroy, and a call it cannot hold returns NSOF_ENOMEM: long sequences are meant to be run in
 * chunks of some hundred frames, each continuing from the previous one's d_ref_out (same stream, bit for bit). */
enum { NSOF_EVENTS_REF_ZERO = 0, NSOF_EVENTS_REF_FIRST = 1, NSOF_EVENTS_REF_GIVEN = 2 };
enum { NSOF_EVENTS_T_FRAME = 0, NSOF_EVENTS_T_LINEAR = 1 };
int nsof_events_from_frames_count_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                      int n, int height, int width, const int64_t* times, const int32_t* lut, int c_on,
                                      int c_off, const int32_t* d_thr_plane, const int32_t* d_ref_in, int ref_mode,
                                      int64_t* frame_bounds_out);
int nsof_events_from_frames_emit_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride, ptrdiff_t frame_stride,
                                     int n, int height, int width, const int64_t* times, const int32_t* lut, int c_on,
                                     int c_off, const int32_t* d_thr_plane, const int32_t* d_ref_in, int ref_mode,
                                     const int64_t* frame_bounds, int timestamps_mode, int p_on, int p_off,
                                     int64_t capacity, int16_t* d_x, int16_t* d_y, int8_t* d_p, int64_t* d_t,
                                     int32_t* d_ref_out);

/* The same generator with two effects of a real sensor: a per-pixel refractory period and
 * background-activity noise events.  Integers only, a counter generator, no atomics: two runs give the same bits and a
 * run cut at any frame equals the one-shot run.  Everything not named here is as above.
 *
 * Per-pixel state besides r: t_ok (int64), the earliest time at which the pixel may fire again; INT64_MIN: never fired
 * (d_t_ok_in NULL starts every pixel there).  The candidates of pixel q = y * width + x at frame k of the call:
 *   signal  the m crossings of the step above with their stamps t_1 <= ... <= t_m (times[k] with _T_FRAME and for frame 0
 *           of a call, else the linear formula).  r moves by m thresholds whether or not the events survive (the
 *           comparator resets, only the read-out is blocked), so d_ref_out does not depend on noise or refractory time.
 *   noise   for k >= 1 only (frame 0 of a call has no interval before it).  One Philox4x32-10 block per pixel and frame:
 *           counter (q, f & 0xffffffff, f >> 32, 0x4E534546) with f = first_frame + k the absolute frame index, key
 *           (seed & 0xffffffff, seed >> 32); outputs c0..c3.  With D = times[k] - times[k-1] and a rate in units of 2^-32
 *           per microsecond, P_on = min(2^32 - 1, rate_on_q * D) in uint64 (likewise P_off): an ON noise event exists iff
 *           c0 < P_on, an OFF one iff c1 < P_off; stamped times[k] (_T_FRAME) or times[k-1] + ((c2 * D) >> 32) (ON) and
 *           the same with c3 (OFF), which lie in [times[k-1], times[k]).  Noise does not move r.  A rate above 1 / D
 *           saturates at one noise event per pixel, polarity and interval.  d_rate_plane != NULL: DEVICE uint32
 *           [height][width][2] (rate_on_q, rate_off_q) per pixel -- hot pixels -- the scalars unused.
 * The candidates of a pixel and frame are walked in the order (t, signal before ON noise before OFF noise), the signal
 * crossings in their own order; a candidate is emitted iff t >= t_ok, and then t_ok = t + refractory_us.  With
 * refractory_us = 0 and no d_t_ok_in nothing is ever dropped.  Stream order as above, a noise event being the last j of
 * its polarity for its pixel and frame; with _T_LINEAR that is the stable sort by t of the order (frame, polarity, y, x, j).
 * The calls over frames [0, k] with first_frame = f and over [k, n) with first_frame = f + k, d_ref_in and d_t_ok_in the
 * first call's d_ref_out and d_t_ok_out, give the one-shot stream, d_ref_out and d_t_ok_out bit for bit.
 *
 * The counts depend on the stamps once candidates can be dropped, so the count entry takes timestamps_mode too, and both
 * entries must be given the same mode and the same *sensor.  sensor == NULL: exactly the entries above (d_t_ok_out is
 * then not written).  d_t_ok_out: DEVICE int64 [height][width], may be d_t_ok_in, may be NULL.
 * NSOF_EINVAL beyond the refusals above, nothing launched and nothing written: refractory_us outside [0, 2^31),
 * first_frame < 0 or first_frame + n beyond 2^62, a timestamps_mode the count entry does not know, a d_t_ok_in without a
 * d_t_ok_out (emit entry), refractory_us > 0 with times[n-1] > INT64_MAX - refractory_us (t_ok = t + refractory_us of a
 * stamp up to times[n-1] would pass the int64 range; the plain entries, which keep no t_ok, take such times, and so do the
 * sensor entries without a refractory time).  A walk through single crossings is needed only with _T_LINEAR and a refractory time or a
 * d_t_ok_in; there a pixel that crosses 2^20 thresholds or more in one step is refused like a bad threshold plane (the
 * count entry returns NSOF_EUNSUPPORTED without filling frame_bounds_out, the emit entry writes nothing). */
typedef struct nsof_events_sensor {
    int64_t refractory_us;        /* [0, 2^31) */
    uint64_t seed;                /* the key of the noise draws */
    int64_t first_frame;          /* the absolute index of frame 0 of this call */
    uint32_t rate_on_q, rate_off_q;   /* noise rates, 2^-32 events per microsecond */
    const uint32_t* d_rate_plane; /* DEVICE [height][width][2] or NULL */
    const int64_t* d_t_ok_in;     /* DEVICE [height][width] or NULL */
} nsof_events_sensor;
int nsof_events_from_frames_sensor_count_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride,
                                             ptrdiff_t frame_stride, int n, int height, int width, const int64_t* times,
                                             const int32_t* lut, int c_on, int c_off, const int32_t* d_thr_plane,
                                             const int32_t* d_ref_in, int ref_mode, int timestamps_mode,
                                             const nsof_events_sensor* sensor, int64_t* frame_bounds_out);
int nsof_events_from_frames_sensor_emit_dev(nsof_ctx* ctx, const uint8_t* d_frames, ptrdiff_t row_stride,
                                            ptrdiff_t frame_stride, int n, int height, int width, const int64_t* times,
                                            const int32_t* lut, int c_on, int c_off, const int32_t* d_thr_plane,
                                            const int32_t* d_ref_in, int ref_mode, const int64_t* frame_bounds,
                                            int timestamps_mode, int p_on, int p_off, int64_t capacity, int16_t* d_x,
                                            int16_t* d_y, int8_t* d_p, int64_t* d_t, int32_t* d_ref_out,
                                            const nsof_events_sensor* sensor, int64_t* d_t_ok_out);
/* The four words c0..c3 of the noise block of (seed, pixel, frame) above, computed on the host: the bits the kernels use. */
void nsof_events_noise_draw(uint64_t seed, uint32_t pixel, int64_t frame, uint32_t* out);

/* Background-activity filter for event streams (csrc/events_denoise.hip): the spatiotemporal
 * correlation filter, in integers throughout.  The stream: d_x, d_y (int16), d_p (int8), d_t (int64), DEVICE arrays of n
 * events, 0 <= n < 2^31, on a height x width sensor; t must not decrease over the stream and may hold any int64 -- the
 * schema and order nsof_events_from_frames_*_dev emit.  State: last, int64 [C][height][width], C = 2 with same_polarity
 * (plane 0 for p > 0, plane 1 otherwise), else 1: the time of the latest event seen at a pixel, INT64_MIN for never.
 * d_last_in NULL: every pixel starts at never.  In stream order, for event i at pixel q of channel c:
 *     lo      = max(t_i - dt_us, INT64_MIN + 1), formed without a wrap
 *     support = the pixels m of the square of `radius` around q, clipped to the sensor, other than q itself unless
 *               include_self, with last_c[m] >= lo
 *     keep_i  = support >= min_support;   then last_c[q] = t_i, kept or not
 * so that a decision depends on the input stream alone.  A run over events [0, k) followed by one over [k, n) from the
 * first one's d_last_out gives the keep bytes, the kept stream and the final last of the one-shot run, bit for bit, for
 * any k; two runs give the same bits (no float, no atomics).
 *
 * The output size depends on the data, so there are two entries.  nsof_events_denoise_mark_dev validates the stream on
 * the device, writes d_keep (uint8 [n], DEVICE: 1 kept, 0 dropped), synchronises and fills the HOST *n_kept_out and, for
 * the n_bounds HOST bounds (non-decreasing, in [0, n]; e.g. the generator's frame_bounds), bounds_out[k] = the kept events
 * before bounds[k] (HOST [n_bounds]): the bounds of the kept stream.  nsof_events_denoise_compact_dev takes d_keep back,
 * validates and counts again on the stream, writes the kept events in input order to d_x_out, d_y_out, d_p_out, d_t_out
 * (DEVICE, `capacity` elements) and the updated state to d_last_out (DEVICE [C][height][width], may be d_last_in, may be
 * NULL); it is asynchronous on the context's stream (only growing the context's workspace waits for it).  The compact pass
 * compares the kept count it has formed itself with `capacity` on the device and writes nothing at all, d_last_out
 * included, unless they are equal and the stream is valid: a keep array of another call cannot send a store past
 * `capacity`.
 * NSOF_EINVAL, nothing launched and nothing written, the value named in nsof_last_error: n outside [0, 2^31), height or
 * width outside [1, 32767], same_polarity or include_self outside {0, 1}, a null stream array or d_keep with n > 0; mark
 * alone: dt_us outside [0, 2^31), radius outside {1, 2}, min_support outside [1, (2 * radius + 1)^2], a null n_kept_out,
 * n_bounds < 0 or above 2^24, bounds without bounds_out, bounds that decrease or leave [0, n]; compact alone: capacity
 * outside [0, n], a null output array with capacity > 0.  A coordinate outside the sensor or a t[i] < t[i-1] is seen on
 * the device only (such an event addresses nothing and supports nothing): the mark entry returns NSOF_EINVAL after its
 * validation pass without writing d_keep, *n_kept_out or bounds_out, the compact entry writes nothing.  n = 0: the mark
 * entry launches nothing and returns zeros, the compact entry only copies the state.
 * Workspace, in the context's workspace, grown on demand and never shrunk before nsof_destroy: about 24 bytes per event
 * -- the words, their sorted copy, and the sort's temporary storage, which holds a third array of n words (the sort is not
 * double-buffered) besides its histograms -- plus 8 bytes per 256 events (the chunk counts) and 8 bytes per bound.
 * Nothing of the sensor's size: the (channel, pixel) segments of the sorted stream are found by binary search, not through
 * a table of offsets.  A call the workspace cannot hold returns NSOF_ENOMEM: run long streams in chunks. */
int nsof_events_denoise_mark_dev(nsof_ctx* ctx, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p, const int64_t* d_t,
                                 int64_t n, int height, int width, int64_t dt_us, int radius, int min_support,
                                 int same_polarity, int include_self, const int64_t* d_last_in, const int64_t* bounds,
                                 int64_t n_bounds, uint8_t* d_keep, int64_t* n_kept_out, int64_t* bounds_out);
int nsof_events_denoise_compact_dev(nsof_ctx* ctx, const int16_t* d_x, const int16_t* d_y, const int8_t* d_p,
                                    const int64_t* d_t, int64_t n, int height, int width, int same_polarity,
                                    const int64_t* d_last_in, const uint8_t* d_keep, int64_t capacity, int16_t* d_x_out,
                                    int16_t* d_y_out, int8_t* d_p_out, int64_t* d_t_out, int64_t* d_last_out);

#ifdef __cplusplus
}
#endif
#endif /* NSOF_H */
