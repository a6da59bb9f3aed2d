// Shape-heterogeneous Farneback batches: the work-list driver.
//
// The reference's gated path calls cv2.calcOpticalFlowFarneback once per ROI, on crops whose shape changes from
// call to call (optical_flow_seg.py:129-164 per connected component, :186-203 union box), and its
// evaluation loop mixes those with full-frame calls (:492-496).  A crop of 520x200 px cannot fill 256 CUs -- the
// fused iteration walks its rows serially in 3 workgroups -- so here MANY such calls share every launch:
//
//   * nsof_farneback_px_batch_desc_dev (this file): per level one launch per stage over a device table of work items
//     (nsof_het_item, nsof_internal.h); an item takes part from its own coarsest level on; the last iteration of
//     level 0 writes straight into the caller's (strided) flow field, so an ROI result lands in the frame-sized
//     canvas without a paste.  Arithmetic per item is that of the per-call path, bit for bit.
//   * nsof_farneback_px_batch (farneback_pipe.hip): the same for HOST memory, as a three-stage pipeline over chunks of
//     the list (upload of chunk c+1 and download of chunk c-1 on their own streams while chunk c computes).
//   * nsof_farneback_px_roi_sequence_dev (farneback_roi.hip): the crops of a gated frame sequence as one such list.
// The other two reach the driver through nsof_farneback_list_core (nsof_internal.h).
// Only the pyramid stage reads frames, so a list of one pixel type differs from a list of another in its pixel size
// (nsof_list_params::src) alone: byte addresses and byte strides throughout, the pyramid kernels' instantiations for the
// type, and for float frames level 0 in the two-kernel form (prep, then expansion).  The typed entries (nsof_farneback_px_*)
// do the work; the nsof_farneback_u8_* and nsof_farneback_f32_* exports at the end of each file name the pixel type and
// forward.
#include <algorithm>
#include <cstring>
#include <vector>

#include "nsof_internal.h"

int nsof_farneback_list_check(nsof_ctx* ctx, int i, const nsof_pair_desc& d, const nsof_list_params& p)
{
    if (!d.prev || !d.next || !d.flow) return nsof_set_error(ctx, NSOF_EINVAL, "pair %d: null pointer", i);
    int rc = nsof_check_farneback_params(ctx, d.width, d.height, p);
    if (rc) return rc;
    if ((rc = nsof_check_frame_layout(ctx, p.src, d.prev, d.prev_stride, 0, d.width, "pair %d prev", i)) ||
        (rc = nsof_check_frame_layout(ctx, p.src, d.next, d.next_stride, 0, d.width, "pair %d next", i)))
        return rc;
    if (!nsof_row_stride_holds(d.prev_stride, d.width, p.src) || !nsof_row_stride_holds(d.next_stride, d.width, p.src))
        return nsof_set_error(ctx, NSOF_EINVAL, "pair %d: row stride < width * %zu", i, p.px());
    if (d.flow_stride < (ptrdiff_t)d.width * 8 || (d.flow_stride & 7) || (reinterpret_cast<uintptr_t>(d.flow) & 7))
        return nsof_set_error(ctx, NSOF_EINVAL, "pair %d: flow stride %lld / pointer must be multiples of 8 bytes and "
                              "the stride >= width*8", i, (long long)d.flow_stride);
    return NSOF_OK;
}

namespace {

// One item through the uniform-shape driver (shapes or parameters the work-list kernels do not cover): frames are
// packed densely, the result is copied into the caller's strided field.
int fallback_item(nsof_ctx* ctx, const nsof_pair_desc& d, const nsof_list_params& p)
{
    const size_t n0 = (size_t)d.width * d.height, row = (size_t)d.width * p.px();
    const size_t szU = align_up(n0 * p.px(), 256), szF = align_up(n0 * 8, 256);
    int rc = ctx->stage.reserve(ctx, 2 * szU + szF);
    if (rc) return rc;
    uint8_t* dP = (uint8_t*)ctx->stage.p;
    uint8_t* dN = dP + szU;
    float* dF = (float*)(dN + szU);
    NSOF_HIP(ctx, hipMemcpy2DAsync(dP, row, d.prev, d.prev_stride, row, d.height, hipMemcpyDeviceToDevice, ctx->stream));
    NSOF_HIP(ctx, hipMemcpy2DAsync(dN, row, d.next, d.next_stride, row, d.height, hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = nsof_farneback_core(ctx, {false, 1, dP, dN, (ptrdiff_t)row, (ptrdiff_t)szU, d.width, d.height, p.src}, dF, p))) return rc;
    NSOF_HIP(ctx, hipMemcpy2DAsync(d.flow, d.flow_stride, dF, (size_t)d.width * 8, (size_t)d.width * 8, d.height,
                                   hipMemcpyDeviceToDevice, ctx->stream));
    return NSOF_OK;
}

// A size class of a level's item table: items [start, start + count) with extents up to max_w x max_h.
struct HetClass {
    int start, count, max_w, max_h;
};

// Sorts a level's items into size classes (power-of-two buckets of width and height).  The tiled kernels of a level
// launch a grid over the LARGEST extents of the items they are given and workgroups outside an item leave at once; with
// one full frame among thousands of small crops nearly every workgroup of such a launch would be one of those (measured:
// 1.9 of 2.0 ms of a level-0 launch), so each class gets its own launch.  Classes with few items share one catch-all.
void sort_into_classes(nsof_het_item* t, int n, std::vector<std::pair<int, int>>& keyed, std::vector<nsof_het_item>& sorted,
                       std::vector<HetClass>& out)
{
    out.clear();
    if (n == 0) return;
    auto bucket = [](int v, int first) {
        int b = 0;
        while (b < 7 && v > (first << b)) b++;
        return b;
    };
    int count[64] = {0};
    keyed.resize(n);
    for (int i = 0; i < n; i++) {
        const int key = bucket(t[i].hk, 16) * 8 + bucket(t[i].wk, 64);
        keyed[i] = {key, i};
        count[key]++;
    }
    // own launch: the 6 most populated buckets with at least 16 items; the rest -> catch-all (key 64)
    int order[64];
    for (int i = 0; i < 64; i++) order[i] = i;
    std::stable_sort(order, order + 64, [&](int a, int b) { return count[a] > count[b]; });
    bool own[64] = {false};
    for (int r = 0; r < 6; r++) own[order[r]] = count[order[r]] >= 16;
    for (auto& kv : keyed)
        if (!own[kv.first]) kv.first = 64;
    std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first < b.first; });
    sorted.resize(n);
    for (int i = 0; i < n; i++) sorted[i] = t[keyed[i].second];
    memcpy(t, sorted.data(), (size_t)n * sizeof(nsof_het_item));
    for (int i = 0; i < n; i++) {
        if (i == 0 || keyed[i].first != keyed[i - 1].first) out.push_back({i, 0, 0, 0});
        HetClass& c = out.back();
        c.count++;
        c.max_w = std::max(c.max_w, t[i].wk);
        c.max_h = std::max(c.max_h, t[i].hk);
    }
}

// The fused iteration kernel's job table of one level (layout: k_iterate_x; *stride = the longest list).  Items go to the
// XCD list with the least work so far, tallest first, the strips of an item one after the other (a strip waits for its
// left neighbour's carries, which must therefore have been taken earlier from the same list).  Returns the number of
// jobs; the table takes 8 + 8 * *stride words.
int build_xjobs(const nsof_het_item* t, int n, unsigned* xj, int* stride, std::vector<std::pair<int, int>>& order,
                std::vector<unsigned> (&lists)[8])
{
    order.resize(n);
    for (int i = 0; i < n; i++) order[i] = {t[i].hk, i};
    std::stable_sort(order.begin(), order.end(), [](const std::pair<int, int>& a, const std::pair<int, int>& b) { return a.first > b.first; });
    long long load[8] = {0};
    for (auto& l : lists) l.clear();
    int jobs = 0;
    for (int r = 0; r < n; r++) {
        const int i = order[r].second;
        const int strips = (t[i].wk + NSOF_X_STRIP - 1) / NSOF_X_STRIP;
        int x = 0;
        for (int k = 1; k < 8; k++)
            if (load[k] < load[x]) x = k;
        for (int s = 0; s < strips; s++) lists[x].push_back((unsigned)i << 8 | (unsigned)s);
        load[x] += (long long)strips * ((t[i].hk + 3) / 4 + 12);   // steps of the walk + a job's start-up
        jobs += strips;
    }
    size_t longest = 1;
    for (auto& l : lists) longest = std::max(longest, l.size());
    for (int k = 0; k < 8; k++) {
        xj[k] = (unsigned)lists[k].size();
        if (!lists[k].empty()) memcpy(xj + 8 + (size_t)k * longest, lists[k].data(), lists[k].size() * sizeof(unsigned));
    }
    *stride = (int)longest;
    return jobs;
}

// A list of equal shapes laid out at constant strides (what the pipelined host entry builds for a video) is the
// uniform batch: it takes that driver and its specialised kernels (decimating pyramid levels, XCD-aware placement).
// Whether descs is one; *f then describes its frames to nsof_farneback_core (the flow fields start at descs[0].flow).
bool uniform_list(int n, const nsof_pair_desc* descs, int src, nsof_fb_frames* f)
{
    if (n < 2) return false;
    const nsof_pair_desc& d0 = descs[0];
    const ptrdiff_t ps = descs[1].prev - d0.prev;
    bool uniform = d0.prev_stride == d0.next_stride && ps > 0 && d0.flow_stride == (ptrdiff_t)d0.width * 8;
    const ptrdiff_t fs = (ptrdiff_t)d0.width * d0.height * 2;   // floats between consecutive dense flow fields
    for (int i = 1; i < n && uniform; i++) {
        const nsof_pair_desc& d = descs[i];
        uniform = d.width == d0.width && d.height == d0.height && d.prev_stride == d0.prev_stride &&
                  d.next_stride == d0.prev_stride && d.flow_stride == d0.flow_stride &&
                  d.prev - d0.prev == (ptrdiff_t)i * ps && d.next - d0.next == (ptrdiff_t)i * ps &&
                  d.flow - d0.flow == (ptrdiff_t)i * fs;
    }
    *f = {false, n, d0.prev, d0.next, d0.prev_stride, ps, d0.width, d0.height, src};
    return uniform;
}

// Items the work-list kernels cover: fused iteration available (window 2..15, >= 1 iteration, at least 2x2 px), and
// at most 255 strips wide (a job of k_iterate_x's table names its strip in 8 bits); wider items run on their own.  The
// Gaussian window has no work-list kernel: every item of such a list runs on its own.
bool het_covers(const nsof_pair_desc& d, const nsof_list_params& p)
{
    return !(p.flags & NSOF_FARNEBACK_GAUSSIAN) && p.iterations >= 1 && nsof_iterate_supported(p.winsize, d.width, d.height) &&
           (d.width + NSOF_X_STRIP - 1) / NSOF_X_STRIP <= 255;
}

// The per-level tables of a work list, as the level loop needs them.
struct HetLevel {
    int count = 0, max_w = 0, max_h = 0;   // items that have this level, and their largest extents
    std::vector<HetClass> classes;
    size_t xj_at = 0;                      // the fused kernel's job table: word offset, list stride, jobs
    int xj_stride = 1, xj_jobs = 0;
};
struct HetPlan {
    int nh = 0;                            // items of the list; level k's table starts at item k * nh
    nsof_iter_form form;
    std::vector<HetLevel> level;           // [0 .. Lmax]
    const nsof_het_item *h_items, *d_items;
    const unsigned* d_xj;
    size_t maxI = 0, maxR = 0, maxF = 0;   // workspace: level images, expansions, one flow buffer (elements)
};

// Item d at level k of its Li levels, but for its workspace offsets.
nsof_het_item het_item(const nsof_pair_desc& d, const nsof_list_params& p, int k, int Li)
{
    nsof_het_item it;
    memset(&it, 0, sizeof(it));
    it.src[0] = d.prev; it.src[1] = d.next;
    it.src_stride[0] = d.prev_stride; it.src_stride[1] = d.next_stride;
    it.out = d.flow;
    it.out_pitch = d.flow_stride / 8;
    it.W = d.width; it.H = d.height;
    nsof_farneback_level_size(d.width, d.height, p.pyr_scale, k, &it.wk, &it.hk, nullptr, nullptr);
    if (k < Li) nsof_farneback_level_size(d.width, d.height, p.pyr_scale, k + 1, &it.pw, &it.ph, nullptr, nullptr);
    const uintptr_t va = 4 * p.px() - 1;   // k_prep_same3_vec's row loads: 4 B (u8) / 8 B (16-bit) / 16 B (f32)
    const bool vec = (d.width & 3) == 0 && d.width >= 8 && (d.prev_stride & va) == 0 && (d.next_stride & va) == 0 &&
                     (reinterpret_cast<uintptr_t>(d.prev) & va) == 0 && (reinterpret_cast<uintptr_t>(d.next) & va) == 0;
    it.flags = vec ? NSOF_HET_VEC0 : 0;
    return it;
}

// Builds and uploads the tables of the items het of descs: per level the item table (sorted into size classes), then the
// fused kernel's job table (8 counts + 8 lists).
int build_plan(nsof_ctx* ctx, const nsof_pair_desc* descs, const std::vector<int>& het, const nsof_list_params& p, HetPlan* plan)
{
    const int nh = plan->nh = (int)het.size();
    // per-item level count; tables per level (items without that level are left out)
    std::vector<int> Li(nh);
    int Lmax = 0;
    long long jobs = 0, strips0 = 0;   // strips of the full-resolution level = the most any level has
    for (int j = 0; j < nh; j++) {
        const nsof_pair_desc& d = descs[het[j]];
        Li[j] = nsof_farneback_effective_levels(d.width, d.height, p.pyr_scale, p.levels);
        Lmax = std::max(Lmax, Li[j]);
        jobs += nsof_iterate_jobs(d.width, d.height);
        strips0 += (d.width + NSOF_X_STRIP - 1) / NSOF_X_STRIP;
    }
    // every item takes a fused form (any of them stands for the list's shape); a list too small to fill the chip
    // with (strip, item) jobs takes the small-batch form of the exact order
    plan->form = nsof_iterate_form(ctx, p.winsize, descs[het[0]].width, descs[het[0]].height, p.iterations, jobs, p.flags);
    const bool use_xj = plan->form == NSOF_ITER_EXACT;   // k_iterate_x runs the list: it needs its job tables
    if (use_xj && (strips0 >= (1ll << 26) || nh >= (1 << 24)))
        return nsof_set_error(ctx, NSOF_EINVAL, "work list too long (%d items, %lld strips)", nh, strips0);
    // words per level at most (every strip in one list)
    const size_t xj_words = use_xj ? align_up(8 + 8 * (size_t)strips0, 64) : 0;
    const size_t items_bytes = align_up((size_t)(Lmax + 1) * nh * sizeof(nsof_het_item), 256);
    // two tables used alternately: the upload of call c may still be queued when call c+1 builds its tables
    const size_t tab_bytes = align_up(items_bytes + (size_t)(Lmax + 1) * xj_words * sizeof(unsigned), 256);
    nsof_table& tab = ctx->het[ctx->het_flip];
    ctx->het_flip ^= 1;
    if (int rc = tab.stage(ctx, tab_bytes, align_up(2 * tab_bytes, 2048))) return rc;
    nsof_het_item* tabs = (nsof_het_item*)tab.h.p;
    unsigned* xj = (unsigned*)((char*)tab.h.p + items_bytes);

    // Build the tables, coarsest level first in memory order k = 0..Lmax (table k at tabs + k*nh).
    plan->level.assign(Lmax + 1, HetLevel());
    std::vector<unsigned> lists[8];
    size_t xj_used = 0;
    std::vector<unsigned long long> offF_prev(nh, 0);   // the item's flow offset at the next coarser level
    std::vector<std::pair<int, int>> keyed;   // (class key, position) scratch
    std::vector<nsof_het_item> sorted;
    for (int k = Lmax; k >= 0; k--) {
        HetLevel& lv = plan->level[k];
        unsigned long long oI = 0, oR = 0, oF = 0;
        nsof_het_item* t = tabs + (size_t)k * nh;
        for (int j = 0; j < nh; j++) {
            if (Li[j] < k) continue;
            nsof_het_item it = het_item(descs[het[j]], p, k, Li[j]);
            const unsigned long long nk = (unsigned long long)it.wk * it.hk;
            it.offI = oI; it.offR = oR; it.offF = oF; it.offFc = offF_prev[j];
            oI += align_up(2 * nk, 64); oR += align_up(10 * nk, 64); oF += align_up(nk, 32);
            offF_prev[j] = it.offF;
            lv.max_w = std::max(lv.max_w, it.wk);
            lv.max_h = std::max(lv.max_h, it.hk);
            t[lv.count++] = it;
        }
        plan->maxI = std::max(plan->maxI, (size_t)oI); plan->maxR = std::max(plan->maxR, (size_t)oR); plan->maxF = std::max(plan->maxF, (size_t)oF);
        sort_into_classes(t, lv.count, keyed, sorted, lv.classes);
        if (use_xj) {
            lv.xj_at = xj_used;
            lv.xj_jobs = build_xjobs(t, lv.count, xj + xj_used, &lv.xj_stride, keyed, lists);
            xj_used += align_up(8 + 8 * (size_t)lv.xj_stride, 64);
        }
    }
    const char* d_tab = (const char*)tab.upload(ctx, items_bytes + xj_used * sizeof(unsigned));
    if (!d_tab) return NSOF_EDEVICE;
    plan->h_items = tabs;
    plan->d_items = (const nsof_het_item*)d_tab;
    plan->d_xj = (const unsigned*)(d_tab + items_bytes);
    return NSOF_OK;
}

// The level loop over a plan.  Workspace: level images, expansions, two flow buffers (every level uses their leading
// part), and for the small-batch form V (column sums, 5 doubles per pixel = the expansion's footprint) and M (matrices, 5
// floats per pixel).
int run_plan(nsof_ctx* ctx, const HetPlan& plan, const nsof_list_params& p, const nsof_poly_taps& ptaps)
{
    const size_t szI = align_up(plan.maxI * 4, 256), szR = align_up(plan.maxR * 4, 256), szF = align_up(plan.maxF * 8, 256);
    const bool lat = plan.form == NSOF_ITER_EXACT_LAT;
    const size_t szV = lat ? szR : 0, szM = lat ? align_up(szR / 2, 256) : 0;
    int rc = ctx->ws.reserve(ctx, szI + szR + 2 * szF + szV + szM);
    if (rc) return rc;
    char* base = (char*)ctx->ws.p;
    float* dI = (float*)base;
    float* dR = (float*)(base + szI);
    float* fb[2] = {(float*)(base + szI + szR), (float*)(base + szI + szR + szF)};
    double* dV = (double*)(base + szI + szR + 2 * szF);
    float* dM = (float*)(base + szI + szR + 2 * szF + szV);
    int cur = 0;
    for (int k = (int)plan.level.size() - 1; k >= 0; k--) {
        const HetLevel& lv = plan.level[k];
        nsof_blur_taps btaps;   // blur taps depend on k only
        if ((rc = nsof_level_geom(ctx, 64, 64, p.pyr_scale, k, nullptr, nullptr, &btaps))) return rc;
        const nsof_het_item* dt = plan.d_items + (size_t)k * plan.nh;
        const nsof_het_item* ht = plan.h_items + (size_t)k * plan.nh;
        // incoming flow of the level (resample of the coarser level's field, zero for items that start here), level
        // image and expansion: grids over the largest extents of a size class, one launch per class
        for (const HetClass& c : lv.classes) {
            if ((rc = nsof_launch_flow_upsample_het(ctx, c.count, dt + c.start, c.max_w, c.max_h, fb[cur],
                                   fb[cur ^ 1], (float)(1. / p.pyr_scale))))
                return rc;
            const bool fused0 = k == 0 && nsof_level0_from_frames(ctx, p.src, btaps);
            const float blur3[2] = {btaps.k[1], btaps.k[2]};
            if (!fused0 && (rc = nsof_launch_prep_het(ctx, c.count, dt + c.start, ht + c.start, k == 0, btaps, dI, p.src)))
                return rc;
            if ((rc = nsof_launch_polyexp_het(ctx, c.count, dt + c.start, c.max_w, c.max_h, ptaps, dI, dR, fused0 ? blur3 : nullptr,
                                              p.src)))
                return rc;
        }
        cur ^= 1;
        for (int it = 0; it < p.iterations; it++) {
            const bool final = k == 0 && it == p.iterations - 1;
            if (lat)
                rc = nsof_launch_iterate_lat_het(ctx, lv.count, dt, lv.max_w, lv.max_h, dR, fb[cur], fb[cur ^ 1], final, p.winsize,
                                                 dM, dV);
            else if (plan.form == NSOF_ITER_EXACT)
                rc = nsof_launch_iterate_x_het(ctx, lv.count, dt, lv.max_w, lv.max_h, dR, szR / 4, fb[cur], fb[cur ^ 1], final,
                                               p.winsize, plan.d_xj + lv.xj_at, lv.xj_stride, lv.xj_jobs);
            else
                rc = nsof_launch_iterate_het(ctx, lv.count, dt, lv.max_w, dR, fb[cur], fb[cur ^ 1], final, p.winsize);
            if (rc) return rc;
            cur ^= 1;
        }
    }
    return NSOF_OK;
}

}  // namespace

// The work-list driver.  descs: HOST array whose pointers are DEVICE addresses.
int nsof_farneback_list_core(nsof_ctx* ctx, int n, const nsof_pair_desc* descs, const nsof_list_params& p)
{
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < n; i++)
        if (int rc = nsof_farneback_list_check(ctx, i, descs[i], p)) return rc;
    nsof_fb_frames uniform;
    if (uniform_list(n, descs, p.src, &uniform)) return nsof_farneback_core(ctx, uniform, descs[0].flow, p);
    std::vector<int> het, rest;
    for (int i = 0; i < n; i++) (het_covers(descs[i], p) ? het : rest).push_back(i);
    if (!het.empty()) {
        nsof_poly_taps ptaps;
        int rc = nsof_host_poly_taps(p.poly_n, p.poly_sigma, &ptaps);
        if (rc) return nsof_set_error(ctx, rc, "poly taps");
        HetPlan plan;
        if ((rc = build_plan(ctx, descs, het, p, &plan)) || (rc = run_plan(ctx, plan, p, ptaps))) return rc;
    }
    for (int i : rest)
        if (int rc = fallback_item(ctx, descs[i], p)) return rc;
    return NSOF_OK;
}

// ---- the work-list routes' entries ------------------------------------------------------------------------------------
extern "C" int nsof_farneback_px_batch_desc_dev(nsof_ctx* ctx, int pixel_type, int n_pairs, const nsof_pair_desc_px* pairs,
                                                double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                                                double poly_sigma, int flags)
{
    if (int rc = nsof_check_typed(ctx, pixel_type)) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return nsof_set_error(ctx, NSOF_EINVAL, "bad pair list");
    if (n_pairs > 32767) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "n_pairs=%d exceeds 32767 per call", n_pairs);
    if (n_pairs == 0) return NSOF_OK;
    const nsof_list_params p(pixel_type, {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags});
    return nsof_farneback_list_core(ctx, n_pairs, reinterpret_cast<const nsof_pair_desc*>(pairs), p);
}

// ---- the 8-bit and float32 exports of these routes: the typed entry with the pixel type named ---------------------------
extern "C" int nsof_farneback_u8_batch_desc_dev(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc* pairs, double pyr_scale,
                                                int levels, int winsize, int iterations, int poly_n, double poly_sigma,
                                                int flags)
{
    return nsof_farneback_px_batch_desc_dev(ctx, NSOF_PIXEL_U8, n_pairs, as_px(pairs), pyr_scale, levels, winsize, iterations,
                                            poly_n, poly_sigma, flags);
}

extern "C" int nsof_farneback_f32_batch_desc_dev(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc_f32* pairs, double pyr_scale,
                                                 int levels, int winsize, int iterations, int poly_n, double poly_sigma,
                                                 int flags)
{
    return nsof_farneback_px_batch_desc_dev(ctx, NSOF_PIXEL_F32, n_pairs, as_px(pairs), pyr_scale, levels, winsize, iterations,
                                            poly_n, poly_sigma, flags);
}
