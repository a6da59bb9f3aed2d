// Internal declarations shared by the HIP translation units of libnsof.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

#include "nsof.h"

#define NSOF_MAX_POLY_N 10    // templated fast kernels exist for radius 1..10 (reference uses 1, 5, 10)
#define NSOF_MAX_BLUR_TAPS 64 // pyramid Gaussian kernel size limit (reference needs <= 19)

struct nsof_prof_slot {
    std::vector<hipEvent_t> start, stop;  // event pool, reused
    size_t used = 0;
    double acc_ms = 0;       // already-collected time
    long long acc_launches = 0;
};

struct nsof_ctx;

// ---- memory the library owns ---------------------------------------------------------------------------------------
// Device memory (Pinned = false) or page-locked host memory on the GPU's NUMA node (Pinned = true) that grows on
// demand and frees itself.  The rule every reuse keeps: memory that a queued copy or kernel may still touch is never
// freed -- reserve() waits on ctx->stream before it lets an old allocation go.
int nsof_buf_grow(nsof_ctx* ctx, bool pinned, void** p, size_t* cap, size_t need, size_t new_cap);
template <class T, bool Pinned> struct nsof_buf {
    T* p = nullptr;
    size_t cap = 0;   // bytes
    nsof_buf() = default;
    nsof_buf(const nsof_buf&) = delete;
    nsof_buf& operator=(const nsof_buf&) = delete;
    ~nsof_buf()
    {
        if (p) (void)(Pinned ? hipHostFree((void*)p) : hipFree((void*)p));
    }
    // At least `need` bytes: an allocation that is smaller is replaced by one of `new_cap` bytes (>= need).
    // NSOF_ENOMEM (set on ctx) if that fails.
    int reserve(nsof_ctx* ctx, size_t need, size_t new_cap) { return nsof_buf_grow(ctx, Pinned, (void**)&p, &cap, need, new_cap); }
    int reserve(nsof_ctx* ctx, size_t need) { return reserve(ctx, need, need); }
    void swap(nsof_buf& o)
    {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
    }
};
template <class T = void> using nsof_dev_buf = nsof_buf<T, false>;
template <class T = void> using nsof_host_buf = nsof_buf<T, true>;

// A table the host writes and one copy uploads: pinned staging, its device copy, and the event after its last upload.
struct nsof_table {
    nsof_host_buf<> h;
    nsof_dev_buf<> d;
    hipEvent_t ev = nullptr;
    ~nsof_table()
    {
        if (ev) (void)hipEventDestroy(ev);
    }
    // `bytes` of host staging at h.p, once the previous upload has left it; a table smaller than `bytes` is replaced
    // (both copies) by one of `cap` bytes.
    int stage(nsof_ctx* ctx, size_t bytes, size_t cap);
    // The first `bytes` of the staging to the device copy on ctx->stream; returns the device copy (nullptr on failure,
    // the error set on ctx: NSOF_EDEVICE).
    const void* upload(nsof_ctx* ctx, size_t bytes);
};

struct nsof_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    unsigned prof_mask = 0;
    nsof_prof_slot prof[NSOF_K_COUNT];
    int opt_polyexp_f32 = 0;   // NSOF_OPT_POLYEXP_F32
    int opt_exact_rowsums = 1; // NSOF_OPT_EXACT_ROWSUMS (default: the library's row-sum order)
    int opt_row_bands = 0;     // NSOF_OPT_ROW_BANDS: 0 off, 1 automatic, >= 4 rows per band
    int opt_small_batch_jobs = 64;    // NSOF_OPT_SMALL_BATCH_JOBS: calls with at most this many (strip, image) jobs take the three-kernel exact form
    int dbg_fault = 0;         // NSOF_OPT_DEBUG_FAULT (test hook): bit 0 k_iterate_x withholds a carry, bit 1 k_lat_colsum a turn
    int opt_pyr_fma = 0;       // NSOF_OPT_PYR_FMA: pyramid blur / resamples with fused multiply-adds (arithmetic variant twin)
    char err[512] = {0};
    // reusable device workspace of the Farneback driver
    nsof_dev_buf<> ws;
    // staging for the host-pointer entry point
    nsof_dev_buf<> stage;
    // pinned host staging of the host-pointer entry point (frames in, flow out)
    nsof_host_buf<> hstage;
    // row-filtered intermediate of the two-pass pyramid kernels
    nsof_dev_buf<> tmp;
    // work-list path: per-level item tables, two used alternately (the pinned copy of one is rewritten two calls later)
    nsof_table het[2];
    int het_flip = 0;
    // pipelined host entry (nsof_farneback_px_batch): copy streams, per-slot staging and events
    struct nsof_pipe* pipe = nullptr;
    // small-batch schedule of the uniform batch driver: a side stream for the pyramid levels and expansions of the
    // finer levels, next to the iterations of the coarser ones, and the events that hand each level over
    hipStream_t side = nullptr;
    std::vector<hipEvent_t> ov_events;
    // private flow buffers of ROI crops that overlap an earlier crop of the same frame pair (nsof_farneback_px_roi_sequence_dev)
    nsof_dev_buf<> roi_tmp;
    // ... and the table of their ordered pastes
    nsof_table paste;
    // box and job tables of the batched segmentation head (nsof_motion_mask_sequence_dev)
    nsof_table seg;
    // im2double table, tap weights and source indices of the Lanczos frame compress (nsof_frames_compress_u8_dev)
    nsof_table frames;
    // per-(trial, cell) parameter planes of the mapped frame-driven run (nsof_accum_frames_f64_maps_dev)
    nsof_table frame_maps;
    // response table and frame times of the event generator (nsof_events_from_frames_*_dev)
    nsof_table events;
    // event streams the accumulators read where they lie in device memory (accum_update.h, "a stream in device memory"):
    // the slice bounds going up, the check's record and the slice tables coming back -- device words and their pinned twin
    nsof_dev_buf<long long> evtab;
    nsof_host_buf<long long> evtab_h;
    // exact-order fused iteration (farneback_iterate_x.hip): strip-to-strip carries (tagged granules, zeroed when
    // allocated, never again: a launch's tag is its epoch), the per-XCD ticket counters + timeout word (x_sync:
    // tickets at word 0, timeout word at word 256), the launch epoch, and whether a launch's timeout word needs a look
    nsof_dev_buf<unsigned long long> x_carry;
    nsof_dev_buf<unsigned> x_sync;
    unsigned x_epoch = 0;
    bool x_dirty = false;
};

int nsof_set_error(nsof_ctx* ctx, int code, const char* fmt, ...);

// ---- run-time value -> template argument ----------------------------------------------------------------------------
// A launcher hands a generic lambda to one of these and instantiates its kernel from the tag the lambda is called with.
// f(std::integral_constant<int, N>{}) for the N in [LO, HI] that equals v; false, f not called, when there is none.
template <int LO, int HI, class Fn>
bool nsof_with_int(int v, Fn&& f)
{
    if constexpr (LO <= HI) {
        if (v != LO) return nsof_with_int<LO + 1, HI>(v, f);
        f(std::integral_constant<int, LO>{});
        return true;
    } else {
        return false;
    }
}
// Page-locked host memory on the GPU's NUMA node (best effort); NUMA node of a device from sysfs, -1 if unknown.
void* nsof_pinned_alloc(int device, size_t bytes);
int nsof_gpu_numa_node(int device);

#define NSOF_HIP(ctx, call)                                                                      \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return nsof_set_error((ctx), NSOF_EDEVICE, "%s failed: %s (%s:%d)", #call,           \
                                  hipGetErrorString(e_), __FILE__, __LINE__);                    \
    } while (0)

// Event bracketing of one launch when profiling of kernel `id` is enabled.
struct nsof_prof_scope {
    nsof_ctx* ctx;
    int id;
    bool on;
    nsof_prof_scope(nsof_ctx* c, int k);
    ~nsof_prof_scope();
};

// ---- Farneback driver pieces shared between farneback_driver.hip and the work-list files (farneback_batch / _pipe / _roi) ----
// Pixel type of the frames a uniform batch reads (the pyramid stage is the only one that reads them).  Frame pointers
// stay byte addresses and every stride stays in bytes for all of them.  The values are those of the public
// nsof_pixel_type.
enum nsof_src_type { NSOF_SRC_U8 = 0, NSOF_SRC_F32 = 1, NSOF_SRC_U16 = 2, NSOF_SRC_S16 = 3 };
static inline int nsof_src_bytes(int src) { return src == NSOF_SRC_F32 ? 4 : (src == NSOF_SRC_U8 ? 1 : 2); }
static inline bool nsof_src_valid(int src) { return src >= NSOF_SRC_U8 && src <= NSOF_SRC_S16; }
// f(nsof_px_tag<T>{}) for the pixel type T of src (an nsof_src_type); false, f not called, for any other value.
template <class T> struct nsof_px_tag { using type = T; };
template <class Fn>
bool nsof_with_src_type(int src, Fn&& f)
{
    switch (src) {
        case NSOF_SRC_U8: f(nsof_px_tag<uint8_t>{}); return true;
        case NSOF_SRC_F32: f(nsof_px_tag<float>{}); return true;
        case NSOF_SRC_U16: f(nsof_px_tag<uint16_t>{}); return true;
        case NSOF_SRC_S16: f(nsof_px_tag<int16_t>{}); return true;
        default: return false;
    }
}
// The first two checks of every typed entry: a context, then a known pixel type.
static inline int nsof_check_typed(nsof_ctx* ctx, int pixel_type)
{
    if (!ctx) return NSOF_EINVAL;
    return nsof_src_valid(pixel_type) ? NSOF_OK : nsof_set_error(ctx, NSOF_EINVAL, "unknown pixel type %d", pixel_type);
}
// The layout rule of a frame (nsof_api.hip): NSOF_EINVAL, the message starting with `who`, unless the start address and
// both strides are multiples of the pixel size and the row stride is at least pixel size * width.
int nsof_check_frame_layout(nsof_ctx* ctx, int src, const void* p, ptrdiff_t row_stride, ptrdiff_t img_stride, int width,
                            const char* who, ...) __attribute__((format(printf, 7, 8)));
// What both drivers ask of a row stride whatever the pixel type (an 8-bit frame has no layout to check): it holds a row.
static inline bool nsof_row_stride_holds(ptrdiff_t row_stride, int width, int src) { return row_stride >= (ptrdiff_t)width * nsof_src_bytes(src); }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// The Farneback parameters as the entry points take them: every typed entry builds this once, everything below passes it on.
struct nsof_fb_params { double pyr_scale; int levels, winsize, iterations, poly_n; double poly_sigma; int flags; };
int nsof_check_farneback_params(nsof_ctx* ctx, int width, int height, const nsof_fb_params& p);
// Frames of the uniform driver: n_pairs independent pairs (prev[i], next[i]), or (sequence) n_pairs + 1 consecutive frames
// in prev, pair i = (frame i, frame i + 1), next unused.  Device BYTE addresses and byte strides whatever the pixel type
// (src: nsof_src_type); pair_stride lies between consecutive frames of either array.
struct nsof_fb_frames {
    bool sequence;
    int n_pairs;
    const uint8_t *prev, *next;
    ptrdiff_t row_stride, pair_stride;
    int width, height, src;
};
// Uniform-shape device batch (farneback_driver.hip); d_flow: n_pairs dense fields.
int nsof_farneback_core(nsof_ctx* ctx, const nsof_fb_frames& frames, float* d_flow, const nsof_fb_params& params);
// What a typed work-list entry was called with (built there): the Farneback parameters and the pixel type of the list (a
// constructor, so that leaving the pixel type out does not compile).
struct nsof_list_params : nsof_fb_params {
    int src;   // nsof_src_type of every frame of the list
    nsof_list_params(int s, const nsof_fb_params& fb) : nsof_fb_params(fb), src(s) {}
    size_t px() const { return (size_t)nsof_src_bytes(src); }   // bytes per pixel
};
// The work-list driver (farneback_batch.hip).  descs: HOST array of n items whose pointers are DEVICE addresses; the
// pipelined host entry (farneback_pipe.hip) and the gated ROI sequence (farneback_roi.hip) hand it their lists.  It checks
// every item with nsof_farneback_list_check, which the host entry also applies to its HOST descriptors before any work
// (`i`: the item's index in the caller's list, for the message).  Hidden, as they were while the three lived in one file:
// the library's dynamic symbol list gains no function.
__attribute__((visibility("hidden"))) int nsof_farneback_list_core(nsof_ctx* ctx, int n, const nsof_pair_desc* descs, const nsof_list_params& p);
__attribute__((visibility("hidden"))) int nsof_farneback_list_check(nsof_ctx* ctx, int i, const nsof_pair_desc& d, const nsof_list_params& p);
// The three descriptor structs of nsof.h have one layout (they differ in the type their frame pointers name); the drivers
// take nsof_pair_desc, whose frame pointers are byte addresses.
template <class D> constexpr bool nsof_is_pair_desc_layout()
{
    return sizeof(D) == sizeof(nsof_pair_desc) && offsetof(D, prev) == offsetof(nsof_pair_desc, prev) &&
           offsetof(D, prev_stride) == offsetof(nsof_pair_desc, prev_stride) && offsetof(D, next) == offsetof(nsof_pair_desc, next) &&
           offsetof(D, next_stride) == offsetof(nsof_pair_desc, next_stride) && offsetof(D, width) == offsetof(nsof_pair_desc, width) &&
           offsetof(D, height) == offsetof(nsof_pair_desc, height) && offsetof(D, flow) == offsetof(nsof_pair_desc, flow) &&
           offsetof(D, flow_stride) == offsetof(nsof_pair_desc, flow_stride);
}
static_assert(nsof_is_pair_desc_layout<nsof_pair_desc_px>(), "nsof_pair_desc_px must keep nsof_pair_desc's layout");
static_assert(nsof_is_pair_desc_layout<nsof_pair_desc_f32>(), "nsof_pair_desc_f32 must keep nsof_pair_desc's layout");
template <class D> static const nsof_pair_desc_px* as_px(const D* pairs) { return reinterpret_cast<const nsof_pair_desc_px*>(pairs); }
void nsof_pipe_destroy(nsof_ctx* ctx);

// ---- Farneback launchers (farneback_pyramid.hip, farneback_resample.hip, farneback_polyexp.hip, farneback_blur.hip) ----
struct nsof_blur_taps {
    int ksize;
    float k[NSOF_MAX_BLUR_TAPS];
};
struct nsof_poly_taps {
    int n;
    float g[NSOF_MAX_POLY_N + 1], xg[NSOF_MAX_POLY_N + 1], xxg[NSOF_MAX_POLY_N + 1];
    double dg[NSOF_MAX_POLY_N + 1], dxxg[NSOF_MAX_POLY_N + 1];
    double ig11, ig03, ig33, ig55;
};

int nsof_host_blur_taps(int ksize, double sigma, nsof_blur_taps* out);
// Size (wk / hk may be null) and pyramid blur taps of a level; on failure the error is set on ctx unless ctx is null.
static inline int nsof_level_geom(nsof_ctx* ctx, int width, int height, double pyr_scale, int level, int* wk, int* hk,
                                  nsof_blur_taps* bt)
{
    int ks;
    double sg;
    int rc = nsof_farneback_level_size(width, height, pyr_scale, level, wk, hk, &ks, &sg);
    if (rc) return ctx ? nsof_set_error(ctx, rc, "bad level geometry") : rc;
    if ((rc = nsof_host_blur_taps(ks, sg, bt)) && ctx)
        return nsof_set_error(ctx, rc, "pyramid blur kernel size %d unsupported (max %d)", ks, NSOF_MAX_BLUR_TAPS - 1);
    return rc;
}
int nsof_host_poly_taps(int n, double sigma, nsof_poly_taps* out);
// Level 0 (the frame's own size, 3-tap smoothing) is formed from the 8- or 16-bit frames by the expansion kernel itself
// (k_polyexp_rs<.., FRAME, SRC>): no pyramid launch, no image written and read back.  Not with the FMA twin of the pyramid
// stages nor with the float expansion (their kernels have no such form), nor for f32 frames: those take the two-kernel
// form (k_prep_same3_vec<.., float>, then the expansion of the level image).  bt: the taps of level 0.
static inline bool nsof_level0_from_frames(const nsof_ctx* ctx, int src, const nsof_blur_taps& bt)
{
    return src != NSOF_SRC_F32 && !ctx->opt_pyr_fma && !ctx->opt_polyexp_f32 && bt.ksize == 3;
}

// ---- shape-heterogeneous work lists (nsof_farneback_px_batch*, nsof_farneback_px_roi_sequence_dev) ----------------
// One work item (a frame pair of its own shape) at ONE pyramid level.  The host builds one table per level (items
// that have no such level are left out) and every stage is launched once per level over the whole table:
// gridDim.z indexes the table (x2 for the per-image stages), gridDim.x/y are sized for the largest item and the
// workgroups outside an item's extent leave at once.  Offsets are element offsets into the level's workspace
// buffers: I (level images, f32; prev at offI, next at offI + wk*hk), R (expansions, f32; R0 at offR, R1 at
// offR + 5*wk*hk), flow (float2; this level at offF, the coarser level's field at offFc).
struct nsof_het_item {
    const uint8_t* src[2];       // full-resolution frames (prev, next), device BYTE addresses: 8-bit, 16-bit or float
                                 // pixels, one type per list (the launch's src_type)
    long long src_stride[2];     // their row strides in bytes
    float* out;                  // the caller's flow field of this item (written by the last iteration of level 0)
    long long out_pitch;         // its row pitch in float2 units
    unsigned long long offI, offR, offF, offFc;
    int W, H;                    // full resolution
    int wk, hk;                  // this level
    int pw, ph;                  // coarser level (0: the item starts here, its incoming flow is zero)
    int flags;                   // NSOF_HET_VEC0 (vector level-0 kernel), W % 4 == 0 and W >= 8 with both frames and their
                                 // row strides 4-byte (8-bit) / 8-byte (16-bit) / 16-byte (float) aligned
    int pad_;
};
enum { NSOF_HET_VEC0 = 1 };

// FarnebackUpdateMatrices (farneback_iterate_lat.hip), the first kernel of the unfused iteration.  R0/R1: the expansions of
// prev/next of pair 0; pair z is at +z*pair_stride floats.
int nsof_launch_update_matrices(nsof_ctx* ctx, int n_pairs, const float* R0, const float* R1, size_t pair_stride,
                                const float* flow, int W, int H, float* M);
// Small-batch exact-order iteration (farneback_iterate_lat.hip): matrices, column sums and row scan as three wide kernels.
// M: 5 floats, V: 5 doubles per pixel of the level (work list: at offR / 2 of each item).  winsize 2..15.
int nsof_launch_iterate_lat(nsof_ctx* ctx, int n_pairs, const float* R0, const float* R1, size_t pair_stride,
                            const float* flow_in, float* flow_out, int W, int H, int winsize, float* M, double* V);
int nsof_launch_iterate_lat_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, int max_h, const float* R,
                                const float* flow_in, float* flow_out, bool final, int winsize, float* M, double* V);
// All launchers are asynchronous on ctx->stream and return an nsof_status.
// The *_het twins take a device table of n_items entries; max_* are the largest extents over the table.
// src_type (nsof_src_type): the pixel type of every item's frames.
int nsof_launch_prep_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, const nsof_het_item* h_items,
                         bool level0, const nsof_blur_taps& taps, float* I, int src_type);
int nsof_launch_polyexp_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, int max_h,
                            const nsof_poly_taps& taps, const float* I, float* R, const float* blur3,
                            int src_type);
int nsof_launch_flow_upsample_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, int max_h,
                                  const float* src, float* dst, float mul);
// final: the flow goes to the items' own output fields (out / out_pitch) instead of flow_out.
int nsof_launch_iterate_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, const float* R,
                            const float* flow_in, float* flow_out, bool final, int winsize);
// The pyramid-level and flow-resample launchers (farneback_pyramid.hip, farneback_resample.hip) take the arithmetic
// variant from ctx->opt_pyr_fma.
// src: n_img frames of pixel type src_type (nsof_src_type), row / image strides in bytes.
int nsof_launch_prep(nsof_ctx* ctx, int n_img, const void* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W,
                     int H, int wk, int hk, const nsof_blur_taps& taps, float* out, int src_type);
// Levels 1..3 of a pyr_scale 0.5 pyramid in one launch; NSOF_EUNSUPPORTED (nothing launched) when the frames do not qualify.
int nsof_launch_prep_decim3(nsof_ctx* ctx, int n_img, const void* src, ptrdiff_t row_stride, ptrdiff_t img_stride, int W,
                            int H, const nsof_blur_taps* taps, float* const* out, int src_type);
int nsof_launch_polyexp(nsof_ctx* ctx, int n_img, const float* img, int W, int H, const nsof_poly_taps& taps,
                        float* R);
// Full-resolution level: pyramid level (3-tap smoothing, centre k0 / side k1) + expansion in one kernel, from the 8-bit
// or 16-bit frames (src_type: not NSOF_SRC_F32).
int nsof_launch_polyexp_frames(nsof_ctx* ctx, int n_img, const void* src0, const void* src1, int nsplit, ptrdiff_t row_stride,
                           ptrdiff_t img_stride, int W, int H, const nsof_poly_taps& taps, float k0, float k1, float* R,
                           int src_type);
int nsof_launch_blur_solve(nsof_ctx* ctx, int n_pairs, const float* M, int W, int H, int winsize, float* flow);
// The same in the reference library's exact summation order; VT: n_pairs * 5 * W * H doubles of scratch.
int nsof_launch_blur_solve_exact(nsof_ctx* ctx, int n_pairs, const float* M, int W, int H, int winsize, double* VT,
                                 float* flow);
// FarnebackUpdateFlow_GaussianBlur (farneback_gauss.hip): separable Gaussian window + solve in one launch, flow in place.
// Windows up to 2 * NSOF_GAUSS_LDS_MAX_M + 1 take the tiled LDS kernel, larger ones (up to 2 * NSOF_GAUSS_MAX_M + 1) a
// slow per-pixel form.  The taps k[0..winsize/2] are formed on the host and passed by value.
#define NSOF_GAUSS_LDS_MAX_M 16
#define NSOF_GAUSS_MAX_M 96
struct nsof_gauss_taps {
    float k[NSOF_GAUSS_MAX_M + 1];
};
int nsof_launch_gauss_blur_solve(nsof_ctx* ctx, int n_pairs, const float* M, int W, int H, int winsize, float* flow);
int nsof_launch_flow_upsample(nsof_ctx* ctx, int n_pairs, const float* src, int sw, int sh, float* dst, int dw,
                              int dh, float mul);
// Fused iteration; flow_in != flow_out.
int nsof_launch_iterate(nsof_ctx* ctx, int n_pairs, const float* R0, const float* R1, size_t pair_stride,
                        const float* flow_in, float* flow_out, int W, int H, int winsize);
// Exact-order fused iteration in ONE kernel (running row sums inside the strip walker, strips chained by carries).
int nsof_launch_iterate_x(nsof_ctx* ctx, int n_pairs, const float* R0, const float* R1, size_t pair_stride,
                          const float* flow_in, float* flow_out, int W, int H, int winsize);
// The same iteration reading its flow_in as resample(coarse_flow [ph][pw][2]) * mul, formed on the fly (k_iterate_xr): what
// nsof_launch_flow_upsample followed by nsof_launch_iterate_x computes, bit for bit, for an exact doubling and the
// two-rounding blend.  NSOF_EUNSUPPORTED, nothing launched, unless W == 2 * pw, H == 2 * ph and winsize is 2..15.
int nsof_launch_iterate_x_resample(nsof_ctx* ctx, int n_pairs, const float* R0, const float* R1, size_t pair_stride,
                                   const float* coarse_flow, int pw, int ph, float mul, float* flow_out, int W, int H,
                                   int winsize);
// d_xjobs: the level's job table -- 8 counts, then 8 lists (one per XCD, `stride` entries apart) of item << 8 | strip;
// njobs = the sum of the counts = the grid; strips are NSOF_X_STRIP output columns wide.
#define NSOF_X_STRIP 192
int nsof_launch_iterate_x_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, int max_h, const float* R,
                              size_t R_floats, const float* flow_in, float* flow_out, bool final, int winsize,
                              const unsigned* d_xjobs, int stride, int njobs);

// ---- the form of the iteration ------------------------------------------------------------------------------------
// The fused kernels (k_iterate_q, k_iterate_x, the small-batch form) take windows 2..15 and need a 2x2 neighbourhood
// for their clamped gather.
static inline bool nsof_iterate_supported(int winsize, int W, int H)
{
    const int m = winsize / 2;
    return m >= 1 && m <= 7 && W >= 2 && H >= 2;
}
// (strip, image) jobs of one W x H image at level 0, what a call is measured by for the small-batch form.  An image whose
// pair the small-batch kernels cannot address with 32-bit byte offsets (40 W H >= 4 GB) counts as more than any call may
// have.
static inline long long nsof_iterate_jobs(int W, int H)
{
    return (unsigned long long)W * H * 40ull < (1ull << 32) ? (W + NSOF_X_STRIP - 1) / NSOF_X_STRIP : 1ll << 31;
}
enum nsof_iter_form {
    NSOF_ITER_FAST,            // fused, per-pixel window sums: k_iterate_q
    NSOF_ITER_EXACT,           // fused, the library's running row sums: k_iterate_x
    NSOF_ITER_EXACT_LAT,       // the same order for small batches: k_update_matrices + k_lat_colsum + k_lat_rowscan
    NSOF_ITER_UNFUSED_FAST,    // k_update_matrices + k_blur_solve
    NSOF_ITER_UNFUSED_EXACT,   // k_update_matrices + k_blur_colsum + k_blur_rowsolve
    NSOF_ITER_UNFUSED_GAUSS,   // k_update_matrices + k_gauss_blur_solve (flags & NSOF_FARNEBACK_GAUSSIAN)
};
// The form every iteration of a call takes, at every level: W x H is level 0, jobs the call's nsof_iterate_jobs summed
// over its pairs.  The exact order is fused only where it iterates; calls of at most NSOF_OPT_SMALL_BATCH_JOBS jobs take
// its small-batch form.  The Gaussian window (flags, as the entry points take them) has one form, whatever the rest says.
static inline nsof_iter_form nsof_iterate_form(const nsof_ctx* ctx, int winsize, int W, int H, int iterations, long long jobs,
                                               int flags)
{
    if (flags & NSOF_FARNEBACK_GAUSSIAN) return NSOF_ITER_UNFUSED_GAUSS;
    const bool fused = nsof_iterate_supported(winsize, W, H);
    if (!ctx->opt_exact_rowsums) return fused ? NSOF_ITER_FAST : NSOF_ITER_UNFUSED_FAST;
    if (!fused || iterations < 1) return NSOF_ITER_UNFUSED_EXACT;
    return jobs <= ctx->opt_small_batch_jobs ? NSOF_ITER_EXACT_LAT : NSOF_ITER_EXACT;
}
static inline bool nsof_form_fused(nsof_iter_form f) { return f <= NSOF_ITER_EXACT_LAT; }
static inline bool nsof_form_exact(nsof_iter_form f) { return f != NSOF_ITER_FAST && f != NSOF_ITER_UNFUSED_FAST; }
// Carry buffer of at least `carry_bytes` (0: whatever exists) + ticket / timeout words of that kernel.
int nsof_xsync_reserve(nsof_ctx* ctx, size_t carry_bytes, unsigned long long** carry, unsigned** tickets, unsigned** err);
// Reads the timeout word of the exact-order kernel after the stream has drained; NSOF_EDEVICE if a carry never arrived.
int nsof_xsync_check(nsof_ctx* ctx);
// hipStreamSynchronize(ctx->stream) + nsof_xsync_check: the tail of every entry point that hands results to the host
int nsof_stream_sync_checked(nsof_ctx* ctx);

// ---- streamed stores ----------------------------------------------------------------------------------------
// Outputs that are not re-read before the caches have turned over (pyramid images, R, flow fields of a batch) are
// written with non-temporal stores: measured on MI355X, the flow resample kernel goes from 3.5 to 6.2 TB/s and the
// level-0 pyramid kernel from 3.7 to 4.4 TB/s (plain stores write-allocate in L2 and evict what the gathers reuse).
#ifdef __HIPCC__
typedef float nsof_f4v __attribute__((ext_vector_type(4)));
typedef float nsof_f2v __attribute__((ext_vector_type(2)));
// 1/x, correctly rounded, for a NORMAL x whose reciprocal is normal too (the determinant + 1e-3 of the 2x2 systems: between
// ~1e-3 and ~1e20 for 8-bit frames).  This is the division sequence the compiler emits for 1./x -- v_rcp_f64, two Newton
// steps, the residual correction of the quotient -- without the operand scaling and special-case fix-ups
// (v_div_scale / v_div_fmas / v_div_fixup: 5 of the 12 instructions) that only matter for subnormal, huge or non-finite
// operands.  Bit-identical to IEEE division on that range (tests/test_farneback_gpu.py::test_recip_matches_ieee_division).
__device__ __forceinline__ double nsof_recip_normal(double x)
{
    double r = __builtin_amdgcn_rcp(x);
    double e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-x, r, 1.0);   // residual of the quotient q0 = 1 * r
    return __builtin_fma(e, r, r);
}

// The 2x2 solve of FarnebackUpdateFlow_Blur for one pixel, from its window sums s0..s4 of the five planes of M and the
// box filter's scale 1 / (winsize * winsize): each sum scaled, the regularised determinant, its reciprocal, the two products.
__device__ __forceinline__ float2 nsof_flow_solve(double s0, double s1, double s2, double s3, double s4, double scale)
{
    const double g11 = s0 * scale, g12 = s1 * scale, g22 = s2 * scale, h1 = s3 * scale, h2 = s4 * scale;
    const double idet = nsof_recip_normal(g11 * g22 - g12 * g12 + 1e-3);
    return make_float2((float)((g11 * h2 - g12 * h1) * idet), (float)((g22 * h1 - g12 * h2) * idet));
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int reflect101(int p, int len)
{
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}
// a * b + c of the pyramid blur and the bilinear resamples in their two arithmetic variants (DESIGN.md section 2,
// NSOF_OPT_PYR_FMA).  FMA = false: multiply, round, add, round, as the library's generic C++ path does (the units are
// compiled with -ffp-contract=off).  FMA = true: one fused multiply-add, the way an AVX2+FMA3 build of the library's vector
// code (v_muladd / v_fma in its separable-filter and resize loops) contracts the same taps in the same order; the leading
// product of a sum is still rounded.
template <bool FMA>
__device__ __forceinline__ float nsof_madd(float a, float b, float c)
{
    if constexpr (FMA) return fmaf(a, b, c);
    else return a * b + c;
}
// cvFloor(float) as its x86-64 build returns it for every float: NaN and
// v >= 2^31 give INT_MIN, v < -2^31 (-inf included) INT_MAX.  A bare (int)v would give 0 for NaN here (v_cvt_i32_f32),
// which sends a NaN flow into the bilinear sample instead of the out-of-image branch.
__device__ __forceinline__ int floor_f(float v)
{
    if (!(v >= -2147483648.0f && v < 2147483648.0f)) return v < 0.f ? 2147483647 : -2147483647 - 1;
    int i = (int)v;
    return i - (i > v);
}
// resize(INTER_LINEAR) coordinate: f = (float)((d+0.5)*scale-0.5); s = floor(f); a = f-s.  The pyramid levels, the flow
// resample (farneback_pyramid.hip, farneback_resample.hip) and the resampling flow source of the exact iteration (iterate_common.h).
__device__ __forceinline__ void lin_coord_x(int d, double scale, int slen, int& s, float& a)
{
    float f = (float)((d + 0.5) * scale - 0.5);
    s = floor_f(f);
    a = f - s;
    if (s < 0) { s = 0; a = 0.f; }
    if (s >= slen - 1) { s = slen - 1; a = 0.f; }
}
__device__ __forceinline__ void lin_coord_y(int d, double scale, int& s, float& a)
{
    float f = (float)((d + 0.5) * scale - 0.5);
    s = floor_f(f);
    a = f - s;
}
// One axis of a bilinear sample as resize takes it: the two source indices and the weight of the second (the first
// gets 1 - w1).  x: the index pair stops at the last column; y: both indices are clamped into the image.
struct LinTap {
    int i0, i1;
    float w1;
};
__device__ __forceinline__ LinTap lin_tap_x(int d, double scale, int len)
{
    LinTap t;
    lin_coord_x(d, scale, len, t.i0, t.w1);
    t.i1 = min(t.i0 + 1, len - 1);
    return t;
}
__device__ __forceinline__ LinTap lin_tap_y(int d, double scale, int len)
{
    LinTap t;
    int s;
    lin_coord_y(d, scale, s, t.w1);
    t.i0 = clampi(s, 0, len - 1);
    t.i1 = clampi(s + 1, 0, len - 1);
    return t;
}
// resize's blend of two samples, p * (1 - w1) + q * w1 in that order, and of 2x2: horizontal first, then vertical.
template <bool FMA>
__device__ __forceinline__ float lin_mix(float p, float q, float w1)
{
    return nsof_madd<FMA>(p, 1.f - w1, q * w1);
}
template <bool FMA>
__device__ __forceinline__ float2 lin_mix(float2 p, float2 q, float w1)
{
    return make_float2(lin_mix<FMA>(p.x, q.x, w1), lin_mix<FMA>(p.y, q.y, w1));
}
template <bool FMA, typename V>
__device__ __forceinline__ V lin_blend(V p00, V p01, V p10, V p11, float a1, float b1)
{
    return lin_mix<FMA>(lin_mix<FMA>(p00, p01, a1), lin_mix<FMA>(p10, p11, a1), b1);
}

// cv2's fixed-point cvtColor to gray of one interleaved 3-channel 8-bit pixel (c0, c1, c2): weights in units of 2^-15,
// w0 on c0 (RGB2GRAY 9798, 19235, 3735; BGR2GRAY 3735, 19235, 9798), rounded.  k_gray_u8 and the pixel-accuracy kernel.
__device__ __forceinline__ unsigned nsof_gray_px(unsigned c0, unsigned c1, unsigned c2, int w0, int w1, int w2)
{
    return (c0 * w0 + c1 * w1 + c2 * w2 + (1u << 14)) >> 15;
}

__device__ __forceinline__ void nsof_store_stream4(float* p, float a, float b, float c, float d)
{
    __builtin_nontemporal_store((nsof_f4v){a, b, c, d}, reinterpret_cast<nsof_f4v*>(p));
}
// (Non-temporal LOADS of the once-read inputs of the iteration kernel were measured too: 3 % slower.)
__device__ __forceinline__ void nsof_store_stream2(float* p, float a, float b)
{
    __builtin_nontemporal_store((nsof_f2v){a, b}, reinterpret_cast<nsof_f2v*>(p));
}
// N = 1, 2, 4 or 8 adjacent floats in the widest streamed stores (p aligned to min(N, 4) floats).
template <int N>
__device__ __forceinline__ void nsof_store_stream_n(float* p, const float (&o)[N])
{
    static_assert(N == 1 || N == 2 || N == 4 || N == 8, "1, 2, 4 or 8 floats");
    if constexpr (N == 1) __builtin_nontemporal_store(o[0], p);
    else if constexpr (N == 2) nsof_store_stream2(p, o[0], o[1]);
    else {
#pragma unroll
        for (int i = 0; i < N; i += 4) nsof_store_stream4(p + i, o[i], o[i + 1], o[i + 2], o[i + 3]);
    }
}

// ---- pyramid-level and flow-resample launchers (farneback_pyramid.hip, farneback_resample.hip) ----------------------
// resize's source step per destination pixel, on the host and for a work item on the device: this double expression,
// which the resample coordinates' bits depend on.
__host__ __device__ inline double inv_scale(int dst, int src) { return 1. / ((double)dst / src); }
// Grid of the kernels that give a 256-thread block 64 x 4 outputs.
static inline dim3 nsof_pixel_grid(int w, int h, int n) { return dim3((w + 63) / 64, (h + 3) / 4, n); }
// f(std::bool_constant<FMA>{}) for the arithmetic variant of the context (NSOF_OPT_PYR_FMA).
template <class Fn>
void nsof_with_fma(const nsof_ctx* ctx, Fn&& f)
{
    if (ctx->opt_pyr_fma) f(std::true_type{});
    else f(std::false_type{});
}
#endif
