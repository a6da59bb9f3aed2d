// The uniform-shape Farneback driver (nsof_farneback_core) and the routes that are nothing but it: device batch, device
// sequence, the lone host pair.  The level loop mirrors the driver of the reference's flow backend
// (cv2.calcOpticalFlowFarneback, called at optical_flow_seg.py:203): coarsest level first, every level resampled from
// the blurred FULL-RES frame.  Host code only: every kernel is behind an nsof_launch_* of its stage's file.
#include <cstdlib>
#include <cstring>

#include "nsof_internal.h"

// Workspace of the uniform driver for B pairs: I [n_img][nk] f32 and R [n_img][5*nk] f32 (level images and
// expansions: one slot that every level reuses, or one slot per level for the latency schedule `lat`), S = second flow
// buffer [B][n0][2], M [B][5][n0] (the unfused forms and the small-batch form), V = column sums [B][5][n0] f64 (the
// unfused and the small-batch exact forms; the Gaussian form has none).  In that order from `base`, sizes in bytes.
struct Carve {
    std::vector<size_t> offI, offR;   // per level, within I / R
    size_t szI = 0, szR = 0, szS = 0, szM = 0, szV = 0;
    char* base = nullptr;             // the workspace, once it is reserved
    size_t total() const { return szI + szR + szS + szM + szV; }
    float* level_I(int k) const { return (float*)(base + offI[k]); }
    float* level_R(int k) const { return (float*)(base + szI + offR[k]); }
    float* S() const { return (float*)(base + szI + szR); }
    float* M() const { return (float*)(base + szI + szR + szS); }
    double* V() const { return (double*)(base + szI + szR + szS + szM); }
};
static Carve farneback_carve(size_t B, bool sequence, int width, int height, double pyr_scale, int L, bool lat,
                             nsof_iter_form form)
{
    Carve c;
    c.offI.assign(L + 1, 0);
    c.offR.assign(L + 1, 0);
    const size_t n0 = (size_t)width * height;
    const size_t n_img = sequence ? B + 1 : 2 * B;   // frames of a sequence, or B prev + B next frames
    for (int k = 0; k <= (lat ? L : 0); k++) {
        int wk, hk;
        nsof_farneback_level_size(width, height, pyr_scale, k, &wk, &hk, nullptr, nullptr);
        c.offI[k] = c.szI;
        c.offR[k] = c.szR;
        c.szI += align_up(n_img * (size_t)wk * hk * 4, 256);
        c.szR += align_up(n_img * 5 * (size_t)wk * hk * 4, 256);
    }
    c.szS = align_up(B * n0 * 8, 256);
    const bool M = form != NSOF_ITER_FAST && form != NSOF_ITER_EXACT;
    const bool V = form == NSOF_ITER_UNFUSED_EXACT || form == NSOF_ITER_EXACT_LAT;
    c.szM = M ? align_up(B * 5 * n0 * 4, 256) : 0;
    c.szV = V ? align_up(B * 5 * n0 * 8, 256) : 0;
    return c;
}

// One run of the level loop -- a batch, or a chunk of one, that fits its workspace -- as its steps share it.
struct Run {
    nsof_ctx* ctx;
    const nsof_fb_frames& f;
    const nsof_fb_params& p;
    int L;                  // the coarsest level
    nsof_iter_form form;
    // Small batches (the three-kernel exact form) take the latency schedule.  A lone call is a chain of ~50 launches that
    // each use a fraction of the chip and cost >= ~5 us (profiles/r03_lone_call_timeline.txt: 762 us at 1080p, a third of
    // it in the two coarsest levels).  Only the FLOW couples the levels; pyramid level and polynomial expansion of every
    // level depend on the input frames alone.  So they move to a side stream (levels L-1 .. 0, into per-level buffers) and
    // run next to the iterations of the coarser levels on the main stream; an event per level hands the expansion over.
    // Same kernels, same arguments, same bits.
    bool lat;
    Carve cv;
    size_t B, n_img;        // pairs, and their frames: B + 1 of a sequence, B prev + B next of a batch
    // A sequence is one array of n_img images.  So are prev and next frames of a batch that lie back to back (the
    // host-pointer entry stages a lone pair that way): one pyramid launch per level instead of two, prev and next apart
    // (a lone call's launches have a ~5 us floor each).  n_first: the images of the first, or only, array.
    int arrays, n_first;
    nsof_poly_taps ptaps;
    float* Ifused[4] = {nullptr, nullptr, nullptr, nullptr};   // level images already made by the three-level launch
};

// Pyramid level + expansion of level k on the current ctx->stream, into the level's slot.
static int level_images(const Run& r, int k, int wk, int hk, const nsof_blur_taps& bt)
{
    const nsof_fb_frames& f = r.f;
    float* Rk = r.cv.level_R(k);
    if (k >= 1 && k <= 3 && r.Ifused[k]) return nsof_launch_polyexp(r.ctx, (int)r.n_img, r.Ifused[k], wk, hk, r.ptaps, Rk);
    if (k == 0 && nsof_level0_from_frames(r.ctx, f.src, bt) && f.width >= 2 && f.height >= 2 && wk == f.width && hk == f.height)
        return nsof_launch_polyexp_frames(r.ctx, (int)r.n_img, f.prev, r.arrays == 1 ? f.prev : f.next, r.n_first, f.row_stride,
                                          f.pair_stride, f.width, f.height, r.ptaps, bt.k[1], bt.k[2], Rk, f.src);
    float* I = r.cv.level_I(k);
    for (int i = 0; i < r.arrays; i++)
        if (int rc = nsof_launch_prep(r.ctx, r.n_first, i == 0 ? f.prev : f.next, f.row_stride, f.pair_stride, f.width, f.height, wk,
                                      hk, bt, I + (size_t)i * r.B * wk * hk, f.src))
            return rc;
    return nsof_launch_polyexp(r.ctx, (int)r.n_img, I, wk, hk, r.ptaps, Rk);
}

// The latency schedule: the coarsest level is needed first and goes to the main stream, levels L-1 .. 0 to the side stream
// with an event after each (ov_events[k]; the level loop waits for it).
static int side_stream_images(const Run& r)
{
    nsof_ctx* ctx = r.ctx;
    const int L = r.L;
    if (!ctx->side) NSOF_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    while (ctx->ov_events.size() < (size_t)(L + 2)) {
        hipEvent_t ev;
        NSOF_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ctx->ov_events.push_back(ev);
    }
    const hipStream_t mainS = ctx->stream, sideS = ctx->side;
    struct Restore { nsof_ctx* cx; hipStream_t saved; ~Restore() { cx->stream = saved; } } restore{ctx, mainS};
    NSOF_HIP(ctx, hipEventRecord(ctx->ov_events[L + 1], mainS));            // the frames are on the device; earlier calls are done
    NSOF_HIP(ctx, hipStreamWaitEvent(sideS, ctx->ov_events[L + 1], 0));
    for (int k = L; k >= 0; k--) {
        int wk, hk;
        nsof_blur_taps bt;
        if (int rc = nsof_level_geom(ctx, r.f.width, r.f.height, r.p.pyr_scale, k, &wk, &hk, &bt)) return rc;
        ctx->stream = k == L ? mainS : sideS;
        if (int rc = level_images(r, k, wk, hk, bt)) return rc;
        if (k < L) NSOF_HIP(ctx, hipEventRecord(ctx->ov_events[k], sideS));
    }
    return NSOF_OK;
}

// pyr_scale 0.5 with three coarser levels (the headline configuration): levels 1..3 smooth and decimate the same
// full-resolution frames -- one launch makes all three (k_prep_decim3), into the level-image buffer that level 0 no longer
// needs before the coarser levels are done with it.  Frames that do not qualify (NSOF_EUNSUPPORTED) are left to the
// per-level path.
static int three_level_images(Run& r)
{
    const nsof_fb_frames& f = r.f;
    nsof_blur_taps bt3[3];
    size_t nk3[3];
    for (int k = 1; k <= 3; k++) {
        int wk, hk;
        if (nsof_level_geom(nullptr, f.width, f.height, r.p.pyr_scale, k, &wk, &hk, &bt3[k - 1]) != 0 ||
            wk * (1 << k) != f.width || hk * (1 << k) != f.height)
            return NSOF_OK;
        nk3[k - 1] = (size_t)wk * hk;
    }
    float* dI = r.cv.level_I(0);
    float* I3[3] = {dI, dI + r.n_img * nk3[0], dI + r.n_img * (nk3[0] + nk3[1])};
    int rc = NSOF_OK;
    for (size_t i = 0; i < (size_t)r.arrays && rc == NSOF_OK; i++) {
        float* I3i[3] = {I3[0] + i * r.B * nk3[0], I3[1] + i * r.B * nk3[1], I3[2] + i * r.B * nk3[2]};
        rc = nsof_launch_prep_decim3(r.ctx, r.n_first, i == 0 ? f.prev : f.next, f.row_stride, f.pair_stride, f.width, f.height, bt3,
                                     I3i, f.src);
    }
    if (rc == NSOF_OK)
        for (int k = 1; k <= 3; k++) r.Ifused[k] = I3[k - 1];
    return rc == NSOF_EUNSUPPORTED ? NSOF_OK : rc;
}

// Does level k's first iteration read the coarser level's flow (pw x ph) itself, resampling it as it fetches
// (nsof_launch_iterate_x_resample), so that the level needs no flow resample launch?  The one-kernel exact form, on an
// exact doubling, with the two-rounding blend; everything else keeps the two kernels.
static bool first_iteration_resamples(const Run& r, int wk, int hk, int pw, int ph)
{
    return r.form == NSOF_ITER_EXACT && r.p.iterations >= 1 && wk == 2 * pw && hk == 2 * ph && !r.ctx->opt_pyr_fma;
}

// The iterations of level k (wk x hk) on the flow in fb[*cur]: the form dispatch and the buffer flips.  A fused iteration
// moves the flow to the other buffer, an unfused one updates it in place.  pw > 0: fb[*cur] still holds the COARSER
// level's flow, pw x ph, and the first iteration resamples it (first_iteration_resamples).
static int iterate_level(const Run& r, int k, int wk, int hk, float* const fb[2], int* cur, int pw, int ph)
{
    nsof_ctx* ctx = r.ctx;
    const int n_pairs = r.f.n_pairs, winsize = r.p.winsize;
    const size_t nk = (size_t)wk * hk;
    // image-major: I [n_img][hk][wk], R [n_img][5*hk*wk].  Pairs: all prev frames then all next frames
    // (R1 = R0 + B images); sequence: the frames in order (R1 = R0 + 1 image).
    const float* R0 = r.cv.level_R(k);
    const float* R1 = R0 + (r.f.sequence ? (size_t)1 : r.B) * 5 * nk;
    float* dM = r.cv.M();
    double* dV = r.cv.V();
    for (int it = 0; it < r.p.iterations; it++) {
        int rc;
        if (nsof_form_fused(r.form)) {
            float* in = fb[*cur];
            float* out = fb[*cur ^= 1];
            if (r.form == NSOF_ITER_EXACT_LAT) rc = nsof_launch_iterate_lat(ctx, n_pairs, R0, R1, 5 * nk, in, out, wk, hk, winsize, dM, dV);
            else if (r.form == NSOF_ITER_EXACT && it == 0 && pw > 0)
                rc = nsof_launch_iterate_x_resample(ctx, n_pairs, R0, R1, 5 * nk, in, pw, ph, (float)(1. / r.p.pyr_scale), out, wk, hk,
                                                    winsize);
            else if (r.form == NSOF_ITER_EXACT) rc = nsof_launch_iterate_x(ctx, n_pairs, R0, R1, 5 * nk, in, out, wk, hk, winsize);
            else rc = nsof_launch_iterate(ctx, n_pairs, R0, R1, 5 * nk, in, out, wk, hk, winsize);
        } else {
            float* flow = fb[*cur];
            if ((rc = nsof_launch_update_matrices(ctx, n_pairs, R0, R1, 5 * nk, flow, wk, hk, dM))) return rc;
            if (r.form == NSOF_ITER_UNFUSED_GAUSS) rc = nsof_launch_gauss_blur_solve(ctx, n_pairs, dM, wk, hk, winsize, flow);
            else if (r.form == NSOF_ITER_UNFUSED_EXACT) rc = nsof_launch_blur_solve_exact(ctx, n_pairs, dM, wk, hk, winsize, dV, flow);
            else rc = nsof_launch_blur_solve(ctx, n_pairs, dM, wk, hk, winsize, flow);
        }
        if (rc) return rc;
    }
    return NSOF_OK;
}

// A run that fits: the schedule of its levels.
static int run_levels(Run& r, float* d_flow)
{
    nsof_ctx* ctx = r.ctx;
    const nsof_fb_frames& f = r.f;
    const int L = r.L, iterations = r.p.iterations;
    int rc = nsof_host_poly_taps(r.p.poly_n, r.p.poly_sigma, &r.ptaps);
    if (rc) return nsof_set_error(ctx, rc, "poly taps");
    if ((rc = ctx->ws.reserve(ctx, r.cv.total()))) return rc;
    r.cv.base = (char*)ctx->ws.p;
    // Two flow buffers, A = the caller's output and S = scratch; every level uses their leading B*nk pixels.
    // Each upsample and each fused iteration moves the flow to the other buffer, so the buffer the coarsest
    // level starts in is chosen such that the last iteration of level 0 writes A.  A level whose first iteration
    // resamples the coarser flow itself has no resample launch, and no flip for one.
    float* const fb[2] = {d_flow, r.cv.S()};
    int flips = nsof_form_fused(r.form) ? L * (1 + iterations) + iterations : L;
    for (int k = L, cw = 0, ch = 0; k >= 0; k--) {   // (cw, ch): level k + 1
        int wk, hk;
        nsof_farneback_level_size(f.width, f.height, r.p.pyr_scale, k, &wk, &hk, nullptr, nullptr);
        if (k < L && first_iteration_resamples(r, wk, hk, cw, ch)) flips--;
        cw = wk;
        ch = hk;
    }
    int cur = flips & 1;

    const hipStream_t mainS = ctx->stream;
    if (r.lat) rc = side_stream_images(r);
    else if (L == 3) rc = three_level_images(r);
    if (rc) return rc;

    int pw = 0, ph = 0;
    for (int k = L; k >= 0; k--) {
        int wk, hk;
        nsof_blur_taps btaps;
        if ((rc = nsof_level_geom(ctx, f.width, f.height, r.p.pyr_scale, k, &wk, &hk, &btaps))) return rc;
        const bool resample_in_first = k < L && first_iteration_resamples(r, wk, hk, pw, ph);
        if (k == L) {
            NSOF_HIP(ctx, hipMemsetAsync(fb[cur], 0, r.B * wk * hk * 8, mainS));
        } else if (!resample_in_first) {
            if ((rc = nsof_launch_flow_upsample(ctx, f.n_pairs, fb[cur], pw, ph, fb[cur ^ 1], wk, hk, (float)(1. / r.p.pyr_scale))))
                return rc;
            cur ^= 1;
        }
        if (!r.lat) {
            if ((rc = level_images(r, k, wk, hk, btaps))) return rc;
        } else if (k < L) {
            NSOF_HIP(ctx, hipStreamWaitEvent(mainS, ctx->ov_events[k], 0));   // this level's expansion is ready
        }
        if ((rc = iterate_level(r, k, wk, hk, fb, &cur, resample_in_first ? pw : 0, ph))) return rc;
        pw = wk;
        ph = hk;
    }
    if (fb[cur] != d_flow)  // cannot happen by construction; keep the result correct regardless
        NSOF_HIP(ctx, hipMemcpyAsync(d_flow, fb[cur], r.B * f.width * f.height * 8, hipMemcpyDeviceToDevice, mainS));
    return NSOF_OK;
}

// How many pairs one run takes.  The unfused exact form keeps 40 B/px of column sums (+ 20 B/px of matrices) in HBM: 64
// pairs of 1920x1080 at a time (8 GB) fill the GPU -- the row walk has one thread per image row.  A batch whose workspace
// would not fit the device's free memory is run in chunks of as many pairs as do fit -- same kernels on sub-ranges of the
// same buffers, so the result does not depend on the chunking.  A batch that fits the workspace already held needs no
// query (lone calls stay cheap).  NSOF_MAX_PAIRS caps the chunk by hand (tests).  Leaves r.cv for a batch of at most *fit.
static int pairs_per_run(Run& r, size_t* fit)
{
    nsof_ctx* ctx = r.ctx;
    auto carve = [&](size_t b) { return farneback_carve(b, r.f.sequence, r.f.width, r.f.height, r.p.pyr_scale, r.L, r.lat, r.form); };
    size_t n = (size_t)r.f.n_pairs;
    if (r.form == NSOF_ITER_UNFUSED_EXACT && n > 64) n = 64;
    r.cv = carve(n);
    if (r.cv.total() > ctx->ws.cap) {
        size_t free_b = 0, total_b = 0;
        NSOF_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        const size_t budget = (size_t)((double)(free_b + ctx->ws.cap) * 0.92);
        size_t lo = 0, hi = n;   // the most pairs whose workspace fits the budget
        while (lo < hi) {
            const size_t mid = (lo + hi + 1) / 2;
            if (carve(mid).total() <= budget) lo = mid;
            else hi = mid - 1;
        }
        n = lo;
    }
    if (const char* e = getenv("NSOF_MAX_PAIRS")) {
        const long v = atol(e);
        if (v >= 1 && (size_t)v < n) n = (size_t)v;
    }
    if (n < 1) n = 1;
    if (n > 32767) n = 32767;   // 2 * pairs images go on gridDim.z of one launch
    *fit = n;
    return NSOF_OK;
}

// Core of every uniform route.  Only the pyramid stage reads the frames.  A batch of more pairs than one run takes
// re-enters in chunks: each chunk chooses its own iteration form from its own pair count (a tail chunk may take the
// small-batch form).  The unfused exact form runs a sequence as its pairs.
int nsof_farneback_core(nsof_ctx* ctx, const nsof_fb_frames& frames, float* d_flow, const nsof_fb_params& p)
{
    if (!ctx) return NSOF_EINVAL;
    nsof_fb_frames f = frames;
    if (f.sequence) f.next = f.prev;
    if (!f.prev || !f.next || !d_flow || f.n_pairs < 1) return nsof_set_error(ctx, NSOF_EINVAL, "null buffer or n_pairs<1");
    int rc = nsof_check_farneback_params(ctx, f.width, f.height, p);
    if (rc) return rc;
    if (!nsof_row_stride_holds(f.row_stride, f.width, f.src))
        return nsof_set_error(ctx, NSOF_EINVAL, "row_stride < width * %d", nsof_src_bytes(f.src));
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const nsof_iter_form form = nsof_iterate_form(ctx, p.winsize, f.width, f.height, p.iterations,
                                                  f.n_pairs * nsof_iterate_jobs(f.width, f.height), p.flags);
    if (form == NSOF_ITER_UNFUSED_EXACT && f.sequence) {
        f.sequence = false;
        f.next = f.prev + f.pair_stride;
    }
    const int L = nsof_farneback_effective_levels(f.width, f.height, p.pyr_scale, p.levels);
    Run r{ctx, f, p, L, form, form == NSOF_ITER_EXACT_LAT && L >= 1};
    size_t fit;
    if ((rc = pairs_per_run(r, &fit))) return rc;
    if ((size_t)f.n_pairs > fit) {
        nsof_fb_frames c = f;
        for (int i = 0; i < f.n_pairs; i += (int)fit) {
            c.n_pairs = f.n_pairs - i < (int)fit ? f.n_pairs - i : (int)fit;
            c.prev = f.prev + (ptrdiff_t)i * f.pair_stride;
            c.next = f.next + (ptrdiff_t)i * f.pair_stride;
            if ((rc = nsof_farneback_core(ctx, c, d_flow + (size_t)i * f.width * f.height * 2, p))) return rc;
        }
        return NSOF_OK;
    }
    r.B = (size_t)f.n_pairs;
    r.n_img = f.sequence ? r.B + 1 : 2 * r.B;
    r.arrays = f.sequence || f.next == f.prev + (ptrdiff_t)f.n_pairs * f.pair_stride ? 1 : 2;
    r.n_first = r.arrays == 1 ? (int)r.n_img : f.n_pairs;
    return run_levels(r, d_flow);
}

// ---- the uniform routes: device batch and device sequence ----------------------------------------------------------
// Every route has ONE typed entry (nsof_pixel_type == nsof_src_type) that does the work, in this order: context, pixel
// type, null pointers and counts, frame layout, then the driver with its parameter checks.  The nsof_farneback_u8* and
// nsof_farneback_f32* exports name the pixel type and forward (the end of this file and of farneback_batch.hip, farneback_pipe.hip, farneback_roi.hip).
extern "C" int nsof_farneback_px_batch_dev(nsof_ctx* ctx, int pixel_type, int n_pairs, const void* d_prev, const void* d_next,
                                           ptrdiff_t row_stride, ptrdiff_t pair_stride, int width, int height, float* d_flow,
                                           double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                                           double poly_sigma, int flags)
{
    if (int rc = nsof_check_typed(ctx, pixel_type)) return rc;
    if (!d_prev || !d_next || !d_flow) return nsof_set_error(ctx, NSOF_EINVAL, "null buffer");
    int rc = nsof_check_frame_layout(ctx, pixel_type, d_prev, row_stride, pair_stride, width, "d_prev");
    if (rc == NSOF_OK) rc = nsof_check_frame_layout(ctx, pixel_type, d_next, row_stride, pair_stride, width, "d_next");
    if (rc) return rc;
    return nsof_farneback_core(ctx, {false, n_pairs, (const uint8_t*)d_prev, (const uint8_t*)d_next, row_stride, pair_stride, width,
                                     height, pixel_type},
                               d_flow, {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags});
}

extern "C" int nsof_farneback_px_sequence_dev(nsof_ctx* ctx, int pixel_type, int n_frames, const void* d_frames,
                                              ptrdiff_t row_stride, ptrdiff_t frame_stride, int width, int height,
                                              float* d_flow, double pyr_scale, int levels, int winsize, int iterations,
                                              int poly_n, double poly_sigma, int flags)
{
    if (int rc = nsof_check_typed(ctx, pixel_type)) return rc;
    if (n_frames < 2) return nsof_set_error(ctx, NSOF_EINVAL, "a sequence needs at least 2 frames");
    if (!d_frames || !d_flow) return nsof_set_error(ctx, NSOF_EINVAL, "null buffer");
    if (int rc = nsof_check_frame_layout(ctx, pixel_type, d_frames, row_stride, frame_stride, width, "d_frames")) return rc;
    return nsof_farneback_core(ctx, {true, n_frames - 1, (const uint8_t*)d_frames, nullptr, row_stride, frame_stride, width, height,
                                     pixel_type},
                               d_flow, {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags});
}

// ---- the lone host pair ----------------------------------------------------------------------------------------------
// src: the pixel type (nsof_src_type).  Dense frames go straight from the caller's memory; strided host views are packed row by row into
// a pinned staging buffer and moved with ONE linear copy per direction: hipMemcpy2D degenerates to a copy per row for
// widths that are not nicely aligned (measured 12 ms for an 801x801 pair against 3 ms of kernels).  On the device the
// pair lies back to back (one pyramid launch per level for both frames).  8-bit frames take any row stride, a flipped
// view's negative one included (nsof_check_frame_layout has nothing to check for them); the parameter checks come
// before the layout check here, so an empty image is NSOF_ESHAPE whatever its strides.
extern "C" int nsof_farneback_px(nsof_ctx* ctx, int src, const void* prev, ptrdiff_t prev_stride, const void* next,
                                 ptrdiff_t next_stride, int width, int height, float* flow, ptrdiff_t flow_stride,
                                 double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                                 double poly_sigma, int flags)
{
    if (int rc = nsof_check_typed(ctx, src)) return rc;
    const nsof_fb_params p{pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags};
    if (!prev || !next || !flow) return nsof_set_error(ctx, NSOF_EINVAL, "null image pointer");
    int rc = nsof_check_farneback_params(ctx, width, height, p);
    if (rc) return rc;
    if ((rc = nsof_check_frame_layout(ctx, src, prev, prev_stride, 0, width, "prev")) ||
        (rc = nsof_check_frame_layout(ctx, src, next, next_stride, 0, width, "next")))
        return rc;
    if (flow_stride < (ptrdiff_t)(width * 8)) return nsof_set_error(ctx, NSOF_EINVAL, "flow_stride < width*8");
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n0 = (size_t)width * height, pitch = (size_t)width * nsof_src_bytes(src);
    const size_t szU = align_up(pitch * height, 256), szF = align_up(n0 * 8, 256);
    if ((rc = ctx->stage.reserve(ctx, 2 * szU + szF)) || (rc = ctx->hstage.reserve(ctx, 2 * szU + szF))) return rc;
    char* hP = (char*)ctx->hstage.p;
    char* hN = hP + szU;
    float* hF = (float*)(hN + szU);
    uint8_t* dP = (uint8_t*)ctx->stage.p;
    uint8_t* dN = dP + szU;
    float* dFl = (float*)(dN + szU);
    const bool in_dense = prev_stride == (ptrdiff_t)pitch && next_stride == (ptrdiff_t)pitch;
    const bool out_dense = flow_stride == (ptrdiff_t)width * 8;
    if (in_dense) {
        NSOF_HIP(ctx, hipMemcpyAsync(dP, prev, pitch * height, hipMemcpyHostToDevice, ctx->stream));
        NSOF_HIP(ctx, hipMemcpyAsync(dN, next, pitch * height, hipMemcpyHostToDevice, ctx->stream));
    } else {
        for (int y = 0; y < height; y++) {
            memcpy(hP + (size_t)y * pitch, (const char*)prev + (ptrdiff_t)y * prev_stride, pitch);
            memcpy(hN + (size_t)y * pitch, (const char*)next + (ptrdiff_t)y * next_stride, pitch);
        }
        NSOF_HIP(ctx, hipMemcpyAsync(dP, hP, 2 * szU, hipMemcpyHostToDevice, ctx->stream));
    }
    if ((rc = nsof_farneback_core(ctx, {false, 1, dP, dN, (ptrdiff_t)pitch, (ptrdiff_t)szU, width, height, src}, dFl, p))) return rc;
    NSOF_HIP(ctx, hipMemcpyAsync(out_dense ? flow : hF, dFl, n0 * 8, hipMemcpyDeviceToHost, ctx->stream));
    // a hand-over between workgroups that never arrived (the exact-order kernels' bounded waits) fails the call, as cv2
    // raises where it fails: the flow of such a launch is never handed back as a result
    if ((rc = nsof_stream_sync_checked(ctx))) return rc;
    if (!out_dense)
        for (int y = 0; y < height; y++)
            memcpy((char*)flow + (ptrdiff_t)y * flow_stride, hF + (size_t)y * width * 2, (size_t)width * 8);
    return NSOF_OK;
}

// ---- the 8-bit and float32 exports of these routes: the typed entry with the pixel type named ---------------------------
extern "C" int nsof_farneback_u8(nsof_ctx* ctx, const uint8_t* prev, ptrdiff_t prev_stride, const uint8_t* next,
                                 ptrdiff_t next_stride, int width, int height, float* flow, ptrdiff_t flow_stride,
                                 double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                                 double poly_sigma, int flags)
{
    return nsof_farneback_px(ctx, NSOF_PIXEL_U8, prev, prev_stride, next, next_stride, width, height, flow, flow_stride,
                             pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
}

extern "C" int nsof_farneback_f32(nsof_ctx* ctx, const float* prev, ptrdiff_t prev_stride, const float* next,
                                  ptrdiff_t next_stride, int width, int height, float* flow, ptrdiff_t flow_stride,
                                  double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                                  double poly_sigma, int flags)
{
    return nsof_farneback_px(ctx, NSOF_PIXEL_F32, prev, prev_stride, next, next_stride, width, height, flow, flow_stride,
                             pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
}

extern "C" int nsof_farneback_u8_batch_dev(nsof_ctx* ctx, int n_pairs, const uint8_t* d_prev, const uint8_t* d_next,
                                           ptrdiff_t row_stride, ptrdiff_t pair_stride, int width, int height,
                                           float* d_flow, double pyr_scale, int levels, int winsize, int iterations,
                                           int poly_n, double poly_sigma, int flags)
{
    return nsof_farneback_px_batch_dev(ctx, NSOF_PIXEL_U8, n_pairs, d_prev, d_next, row_stride, pair_stride, width, height,
                                       d_flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
}

extern "C" int nsof_farneback_f32_batch_dev(nsof_ctx* ctx, int n_pairs, const float* d_prev, const float* d_next,
                                            ptrdiff_t row_stride, ptrdiff_t pair_stride, int width, int height,
                                            float* d_flow, double pyr_scale, int levels, int winsize, int iterations,
                                            int poly_n, double poly_sigma, int flags)
{
    return nsof_farneback_px_batch_dev(ctx, NSOF_PIXEL_F32, n_pairs, d_prev, d_next, row_stride, pair_stride, width, height,
                                       d_flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
}

extern "C" int nsof_farneback_u8_sequence_dev(nsof_ctx* ctx, int n_frames, const uint8_t* d_frames,
                                              ptrdiff_t row_stride, ptrdiff_t frame_stride, int width, int height,
                                              float* d_flow, double pyr_scale, int levels, int winsize,
                                              int iterations, int poly_n, double poly_sigma, int flags)
{
    return nsof_farneback_px_sequence_dev(ctx, NSOF_PIXEL_U8, n_frames, d_frames, row_stride, frame_stride, width, height,
                                          d_flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
}

extern "C" int nsof_farneback_f32_sequence_dev(nsof_ctx* ctx, int n_frames, const float* d_frames,
                                               ptrdiff_t row_stride, ptrdiff_t frame_stride, int width, int height,
                                               float* d_flow, double pyr_scale, int levels, int winsize,
                                               int iterations, int poly_n, double poly_sigma, int flags)
{
    return nsof_farneback_px_sequence_dev(ctx, NSOF_PIXEL_F32, n_frames, d_frames, row_stride, frame_stride, width, height,
                                          d_flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags);
}
