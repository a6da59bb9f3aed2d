// The pipelined host entry of the Farneback work lists (nsof_farneback_px_batch): frames and flow fields in HOST memory,
// as a three-stage pipeline over chunks of the list -- upload of chunk c+1 and download of chunk c-1 on their own streams
// while chunk c computes in the work-list driver (nsof_farneback_list_core, farneback_batch.hip).  Page-locked frames and
// flow fields are copied directly; pageable or strided ones go through the page-locked staging of one of three slots,
// packed and unpacked by a few threads on the GPU's NUMA node.
#include <sched.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "nsof_internal.h"

namespace {

// CPUs of a NUMA node (sysfs cpulist "0-63,128-191"), empty if unknown.
std::vector<int> node_cpus(int node)
{
    std::vector<int> out;
    if (node < 0) return out;
    char path[96];
    snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
    FILE* f = fopen(path, "r");
    if (!f) return out;
    int a, b;
    char sep;
    while (fscanf(f, "%d", &a) == 1) {
        b = a;
        if (fscanf(f, "%c", &sep) == 1 && sep == '-') {
            if (fscanf(f, "%d", &b) != 1) b = a;
            if (fscanf(f, "%c", &sep) != 1) sep = 0;
        }
        for (int c = a; c <= b; c++) out.push_back(c);
        if (sep != ',') break;
    }
    fclose(f);
    return out;
}

thread_local int g_pack_node = -1;   // NUMA node the packing threads of THIS calling thread prefer (set per call from the context's device)

void parallel_rows(size_t n_tasks, const std::function<void(size_t)>& fn)
{
    static const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const unsigned nt = (unsigned)std::min<size_t>(std::min(16u, std::max(1u, hw / 2)), n_tasks);
    if (nt <= 1) {
        for (size_t i = 0; i < n_tasks; i++) fn(i);
        return;
    }
    static thread_local std::vector<int> cpus;
    static thread_local int cpus_node = -2;
    if (cpus_node != g_pack_node) {
        cpus = node_cpus(g_pack_node);
        cpus_node = g_pack_node;
    }
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t] {
            if (!cpus.empty()) {   // the staging buffers live on the GPU's node: copy from there (best effort)
                cpu_set_t set;
                CPU_ZERO(&set);
                for (int c : cpus)
                    if (c < CPU_SETSIZE) CPU_SET(c, &set);
                (void)sched_setaffinity(0, sizeof(set), &set);
            }
            for (size_t i = t; i < n_tasks; i += nt) fn(i);
        });
    for (auto& x : th) x.join();
}

}  // namespace

struct __attribute__((visibility("hidden"))) nsof_pipe {   // hidden: its destructor is no symbol of the library
    hipStream_t s_in = nullptr, s_out = nullptr;
    struct Slot {
        nsof_dev_buf<> d_in, d_out;
        nsof_host_buf<> h_in, h_out;
        hipEvent_t in_done = nullptr, compute_done = nullptr, out_done = nullptr;
    } slot[3];
    static constexpr int NSLOT = 3;
    ~nsof_pipe()
    {
        for (auto& s : slot) {
            if (s.in_done) hipEventDestroy(s.in_done);
            if (s.compute_done) hipEventDestroy(s.compute_done);
            if (s.out_done) hipEventDestroy(s.out_done);
        }
        if (s_in) hipStreamDestroy(s_in);
        if (s_out) hipStreamDestroy(s_out);
    }
};

void nsof_pipe_destroy(nsof_ctx* ctx)
{
    delete ctx->pipe;
    ctx->pipe = nullptr;
}

namespace {

// The context's pipe, built on first use: built completely, then stored.  A stream or event that cannot be created ends
// the call (the error set on ctx), what was made is destroyed with the local, and the context still holds no pipe.
int pipe_get(nsof_ctx* ctx, nsof_pipe** out)
{
    if (!ctx->pipe) {
        std::unique_ptr<nsof_pipe> p(new (std::nothrow) nsof_pipe());
        if (!p) return nsof_set_error(ctx, NSOF_ENOMEM, "out of host memory");
        NSOF_HIP(ctx, hipStreamCreateWithFlags(&p->s_in, hipStreamNonBlocking));
        NSOF_HIP(ctx, hipStreamCreateWithFlags(&p->s_out, hipStreamNonBlocking));
        for (auto& s : p->slot) {
            NSOF_HIP(ctx, hipEventCreateWithFlags(&s.in_done, hipEventDisableTiming));
            NSOF_HIP(ctx, hipEventCreateWithFlags(&s.compute_done, hipEventDisableTiming));
            NSOF_HIP(ctx, hipEventCreateWithFlags(&s.out_done, hipEventDisableTiming));
        }
        ctx->pipe = p.release();
    }
    *out = ctx->pipe;
    return NSOF_OK;
}

// Pinned (page-locked, HIP-registered) host memory can be the source / target of an asynchronous copy directly.
bool is_pinned(const void* p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();   // not a HIP allocation: clear the sticky error
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

// ---- the chunk plan ---------------------------------------------------------------------------------------------------
// A chunk of the list, planned once.  Vectors are indexed by i - lo.  A frame or flow field is "direct" when it is dense
// and page-locked: the copy engine reads or writes the caller's memory; every other one goes through the slot's staging.
struct Chunk {
    int lo, hi;                       // items [lo, hi)
    std::vector<size_t> in_off[2];    // byte offsets of the packed frames in the slot's input buffer
    std::vector<size_t> out_off;      // byte offsets of the dense flow fields in the slot's output buffer
    std::vector<char> direct_in[2], direct_out;
    size_t in_bytes = 0, out_bytes = 0;
    int n_direct_in = 0, n_direct_out = 0;   // how many frames (of 2 per item) / flow fields are direct
    int items() const { return hi - lo; }
    bool bulk_in() const { return n_direct_in == 0; }           // every frame is packed: one upload out of the staging
    bool bulk_out() const { return n_direct_out == 0; }         // every flow field is staged: one download into the staging
    bool staged_out() const { return n_direct_out < items(); }  // some flow field needs h_out and an unpack afterwards
};

const uint8_t* frame_of(const nsof_pair_desc& d, int f) { return f ? d.next : d.prev; }
ptrdiff_t frame_stride_of(const nsof_pair_desc& d, int f) { return f ? d.next_stride : d.prev_stride; }

// Bytes of flow per chunk: about 512 MiB (32 pairs of 1920x1080) -- small enough that upload, compute and download of
// neighbouring chunks overlap for lists of a hundred frames, large enough that the work list of a chunk still fills the
// GPU (the download, not the compute, bounds the pipeline: 16.6 MB per 1080p pair).
size_t chunk_budget(int n_pairs, const nsof_pair_desc* pairs)
{
    if (const char* chunk_env = getenv("NSOF_PIPE_CHUNK_MB"))   // tests shrink it to force several chunks
        return (size_t)std::max(1l, atol(chunk_env)) << 20;
    // about 16 chunks per list, so that the pipeline's fill and drain (one upload + compute before the first
    // download, one download after the last compute) stay a small share: measured at 256 pairs of 1080p, 256 MiB
    // chunks 2.78 k pairs/s, 512 MiB 2.61 k, 128 MiB 2.15 k (8-pair work lists no longer fill the GPU)
    size_t total_out = 0;
    for (int i = 0; i < n_pairs; i++) total_out += (size_t)pairs[i].width * pairs[i].height * 8;
    return std::min<size_t>(512u << 20, std::max<size_t>(256u << 20, total_out / 16));
}

// The chunks of a list: a chunk closes once it holds the budget of flow (or 8192 items).
std::vector<Chunk> plan_chunks(int n_pairs, const nsof_pair_desc* pairs, const nsof_list_params& p)
{
    const size_t budget = chunk_budget(n_pairs, pairs);
    std::vector<Chunk> chunks;
    for (int i = 0; i < n_pairs;) {
        Chunk c;
        c.lo = i;
        for (; i < n_pairs && (i == c.lo || (c.out_bytes < budget && i - c.lo < 8192)); i++) {
            const nsof_pair_desc& d = pairs[i];
            const size_t n0 = (size_t)d.width * d.height;
            for (int f = 0; f < 2; f++) {
                const bool direct = frame_stride_of(d, f) == (ptrdiff_t)(d.width * p.px()) && is_pinned(frame_of(d, f));
                c.in_off[f].push_back(c.in_bytes);
                c.direct_in[f].push_back(direct);
                c.in_bytes += align_up(n0 * p.px(), 256);
                c.n_direct_in += direct;
            }
            const bool direct = d.flow_stride == (ptrdiff_t)d.width * 8 && is_pinned(d.flow);
            c.out_off.push_back(c.out_bytes);
            c.direct_out.push_back(direct);
            c.out_bytes += align_up(n0 * 8, 256);
            c.n_direct_out += direct;
        }
        c.hi = i;
        chunks.push_back(std::move(c));
    }
    return chunks;
}

// ---- NSOF_PIPE_TRACE ---------------------------------------------------------------------------------------------------
// NSOF_PIPE_TRACE=1: device-side begin/end of every stage of every chunk (timing events) and the host's packing times,
// printed at the end of a call that succeeds.  The trace owns its events.
struct Trace {
    enum { H2D_BEGIN, H2D_END, COMPUTE_BEGIN, COMPUTE_END, D2H_BEGIN, D2H_END, N_MARKS };
    const bool on = getenv("NSOF_PIPE_TRACE") != nullptr;
    std::vector<std::array<hipEvent_t, N_MARKS>> ev;
    std::vector<std::array<double, 2>> pack;   // host time at the begin / end of packing, ms from the call
    const double t_call = now_ms();
    explicit Trace(int n_chunks) : ev(on ? n_chunks : 0, std::array<hipEvent_t, N_MARKS>{}), pack(on ? n_chunks : 0) {}
    Trace(const Trace&) = delete;
    ~Trace()
    {
        for (auto& a : ev)
            for (auto e : a)
                if (e) (void)hipEventDestroy(e);
    }
    static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void mark(int ci, int k, hipStream_t st)
    {
        if (!on) return;
        hipEventCreate(&ev[ci][k]);
        hipEventRecord(ev[ci][k], st);
    }
    void pack_mark(int ci, int k)
    {
        if (on) pack[ci][k] = now_ms() - t_call;
    }
    void print(const std::vector<Chunk>& chunks) const
    {
        if (!on) return;
        const int nc = (int)chunks.size();
        fprintf(stderr, "[nsof pipe] %d chunks, host total %.2f ms; per chunk: pairs | host pack begin..end | h2d | compute | d2h (ms from first upload)\n",
                nc, now_ms() - t_call);
        for (int ci = 0; ci < nc; ci++) {
            float t[N_MARKS];
            for (int k = 0; k < N_MARKS; k++) hipEventElapsedTime(&t[k], ev[0][0], ev[ci][k]);
            fprintf(stderr, "[nsof pipe] %3d: %4d | %7.2f..%7.2f | %7.2f..%7.2f | %7.2f..%7.2f | %7.2f..%7.2f\n", ci,
                    chunks[ci].items(), pack[ci][0], pack[ci][1], t[0], t[1], t[2], t[3], t[4], t[5]);
        }
    }
};

// ---- one call of the pipelined entry -----------------------------------------------------------------------------------
// The steps a chunk goes through, in the order the chunk loop of batch_host takes them.  Chunk ci uses slot ci % NSLOT,
// which carried chunk ci - NSLOT before ("reuse").
struct PipeRun {
    nsof_ctx* ctx;
    nsof_pipe* pp;
    const nsof_pair_desc* pairs;
    const nsof_list_params& p;
    const std::vector<Chunk> chunks;
    std::vector<char> unpacked;          // per chunk: its flows have reached the caller's memory
    std::vector<nsof_pair_desc> dd;      // device descriptors of the chunk being queued
    Trace trace;
    const char* const fail_env = getenv("NSOF_PIPE_FAIL_AFTER_CHUNK");   // tests: the chunk after whose compute the call fails
    const int fail_after = fail_env ? atoi(fail_env) : -1;

    PipeRun(nsof_ctx* c, nsof_pipe* pipe, int n_pairs, const nsof_pair_desc* list, const nsof_list_params& params)
        : ctx(c), pp(pipe), pairs(list), p(params), chunks(plan_chunks(n_pairs, list, params)), unpacked(chunks.size(), 0),
          trace((int)chunks.size())
    {
    }
    nsof_pipe::Slot& slot(int ci) const { return pp->slot[ci % nsof_pipe::NSLOT]; }
    static bool reuse(int ci) { return ci >= nsof_pipe::NSLOT; }

    // Flows of a finished chunk -> the caller's memory (the staged ones; the direct ones are there once out_done is).
    int unpack(int ci)
    {
        const Chunk& c = chunks[ci];
        nsof_pipe::Slot& s = slot(ci);
        NSOF_HIP(ctx, hipEventSynchronize(s.out_done));
        std::vector<std::pair<int, int>> rows;   // (item, first row) tasks of 64 rows
        for (int i = c.lo; i < c.hi; i++)
            if (!c.direct_out[i - c.lo])
                for (int y = 0; y < pairs[i].height; y += 64) rows.emplace_back(i, y);
        parallel_rows(rows.size(), [&](size_t t) {
            const int i = rows[t].first, y0 = rows[t].second;
            const nsof_pair_desc& d = pairs[i];
            const char* src = (const char*)s.h_out.p + c.out_off[i - c.lo];
            for (int y = y0; y < std::min(y0 + 64, d.height); y++)
                memcpy((char*)d.flow + (ptrdiff_t)y * d.flow_stride, src + (size_t)y * d.width * 8, (size_t)d.width * 8);
        });
        unpacked[ci] = 1;
        return NSOF_OK;
    }

    // Host-side waits only where host memory is reused: the slot's pinned input staging (its upload has long
    // finished) and, for pageable outputs, its pinned output staging (must be unpacked before the next download
    // lands in it; a buffer that has to grow for chunk ci must have been left by the old download too).  Everything
    // else is ordered on the GPU by events, so the host runs ahead and packs.
    int wait_for_slot(int ci)
    {
        if (!reuse(ci)) return NSOF_OK;
        const Chunk &c = chunks[ci], &before = chunks[ci - nsof_pipe::NSLOT];
        nsof_pipe::Slot& s = slot(ci);
        NSOF_HIP(ctx, hipEventSynchronize(s.in_done));
        const bool grows = s.h_out.cap < c.out_bytes || s.d_out.cap < c.out_bytes || s.d_in.cap < c.in_bytes || s.h_in.cap < c.in_bytes;
        if (!unpacked[ci - nsof_pipe::NSLOT] && (before.staged_out() || grows)) return unpack(ci - nsof_pipe::NSLOT);
        return NSOF_OK;
    }

    int reserve(int ci)
    {
        const Chunk& c = chunks[ci];
        nsof_pipe::Slot& s = slot(ci);
        int rc;
        if ((rc = s.d_in.reserve(ctx, c.in_bytes)) || (rc = s.d_out.reserve(ctx, c.out_bytes)) || (rc = s.h_in.reserve(ctx, c.in_bytes)) ||
            (c.staged_out() && (rc = s.h_out.reserve(ctx, c.out_bytes))))
            return rc;
        return NSOF_OK;
    }

    // Pageable / strided frames of a chunk -> the slot's pinned input staging, by a few threads.
    void pack(int ci)
    {
        const Chunk& c = chunks[ci];
        nsof_pipe::Slot& s = slot(ci);
        trace.pack_mark(ci, 0);
        std::vector<std::array<int, 3>> rows;   // (item, frame, first row)
        for (int i = c.lo; i < c.hi; i++)
            for (int f = 0; f < 2; f++)
                if (!c.direct_in[f][i - c.lo])
                    for (int y = 0; y < pairs[i].height; y += 128) rows.push_back({i, f, y});
        parallel_rows(rows.size(), [&](size_t t) {
            const int i = rows[t][0], f = rows[t][1], y0 = rows[t][2];
            const nsof_pair_desc& d = pairs[i];
            const uint8_t* src = frame_of(d, f);
            const ptrdiff_t st = frame_stride_of(d, f);
            uint8_t* dst = (uint8_t*)s.h_in.p + c.in_off[f][i - c.lo];
            const int y1 = std::min(y0 + 128, d.height);
            const size_t row = (size_t)d.width * p.px();   // bytes of a packed row
            if (st == (ptrdiff_t)row) {
                memcpy(dst + (size_t)y0 * row, src + (ptrdiff_t)y0 * st, (size_t)(y1 - y0) * row);
            } else {
                for (int y = y0; y < y1; y++) memcpy(dst + (size_t)y * row, src + (ptrdiff_t)y * st, row);
            }
        });
        trace.pack_mark(ci, 1);
    }

    // Stage 1: frames -> device on s_in.  One copy when every frame was packed, otherwise one per frame from the frame's
    // own memory or its place in the staging.
    int upload(int ci)
    {
        const Chunk& c = chunks[ci];
        nsof_pipe::Slot& s = slot(ci);
        if (reuse(ci)) NSOF_HIP(ctx, hipStreamWaitEvent(pp->s_in, s.compute_done, 0));   // d_in was read by chunk ci - NSLOT
        trace.mark(ci, Trace::H2D_BEGIN, pp->s_in);
        if (c.bulk_in()) {
            NSOF_HIP(ctx, hipMemcpyAsync(s.d_in.p, s.h_in.p, c.in_bytes, hipMemcpyHostToDevice, pp->s_in));
        } else {
            for (int i = c.lo; i < c.hi; i++)
                for (int f = 0; f < 2; f++) {
                    const size_t off = c.in_off[f][i - c.lo], n0 = (size_t)pairs[i].width * pairs[i].height * p.px();
                    const void* src = c.direct_in[f][i - c.lo] ? (const void*)frame_of(pairs[i], f) : (const void*)((char*)s.h_in.p + off);
                    NSOF_HIP(ctx, hipMemcpyAsync((char*)s.d_in.p + off, src, n0, hipMemcpyHostToDevice, pp->s_in));
                }
        }
        NSOF_HIP(ctx, hipEventRecord(s.in_done, pp->s_in));
        trace.mark(ci, Trace::H2D_END, pp->s_in);
        return NSOF_OK;
    }

    // The chunk as a list of the work-list driver: dense frames and flow fields in the slot's device buffers.
    void device_descs(const Chunk& c, const nsof_pipe::Slot& s)
    {
        dd.resize(c.items());
        for (int i = c.lo; i < c.hi; i++) {
            nsof_pair_desc& d = dd[i - c.lo];
            d.prev = (const uint8_t*)s.d_in.p + c.in_off[0][i - c.lo];
            d.next = (const uint8_t*)s.d_in.p + c.in_off[1][i - c.lo];
            d.prev_stride = d.next_stride = (ptrdiff_t)(pairs[i].width * p.px());
            d.width = pairs[i].width;
            d.height = pairs[i].height;
            d.flow = (float*)((char*)s.d_out.p + c.out_off[i - c.lo]);
            d.flow_stride = (ptrdiff_t)pairs[i].width * 8;
        }
    }

    // Stage 2: compute on the context's stream.
    int compute(int ci)
    {
        const Chunk& c = chunks[ci];
        nsof_pipe::Slot& s = slot(ci);
        NSOF_HIP(ctx, hipStreamWaitEvent(ctx->stream, s.in_done, 0));
        if (reuse(ci)) NSOF_HIP(ctx, hipStreamWaitEvent(ctx->stream, s.out_done, 0));   // d_out is being downloaded (chunk ci - NSLOT)
        device_descs(c, s);
        trace.mark(ci, Trace::COMPUTE_BEGIN, ctx->stream);
        if (int rc = nsof_farneback_list_core(ctx, c.items(), dd.data(), p)) return rc;
        if (fail_after >= 0 && ci == fail_after)   // NSOF_PIPE_FAIL_AFTER_CHUNK (tests): an error with copies in flight
            return nsof_set_error(ctx, NSOF_ENOMEM, "NSOF_PIPE_FAIL_AFTER_CHUNK=%d: injected failure", fail_after);
        NSOF_HIP(ctx, hipEventRecord(s.compute_done, ctx->stream));
        trace.mark(ci, Trace::COMPUTE_END, ctx->stream);
        return NSOF_OK;
    }

    // Stage 3: flow -> host on s_out.  One copy when every flow field is staged, otherwise one per field into the field's
    // own memory or its place in the staging.
    int download(int ci)
    {
        const Chunk& c = chunks[ci];
        nsof_pipe::Slot& s = slot(ci);
        NSOF_HIP(ctx, hipStreamWaitEvent(pp->s_out, s.compute_done, 0));
        trace.mark(ci, Trace::D2H_BEGIN, pp->s_out);
        if (c.bulk_out()) {
            NSOF_HIP(ctx, hipMemcpyAsync(s.h_out.p, s.d_out.p, c.out_bytes, hipMemcpyDeviceToHost, pp->s_out));
        } else {
            for (int i = c.lo; i < c.hi; i++) {
                const size_t off = c.out_off[i - c.lo], nb = (size_t)pairs[i].width * pairs[i].height * 8;
                void* dst = c.direct_out[i - c.lo] ? (void*)pairs[i].flow : (void*)((char*)s.h_out.p + off);
                NSOF_HIP(ctx, hipMemcpyAsync(dst, (char*)s.d_out.p + off, nb, hipMemcpyDeviceToHost, pp->s_out));
            }
        }
        NSOF_HIP(ctx, hipEventRecord(s.out_done, pp->s_out));
        trace.mark(ci, Trace::D2H_END, pp->s_out);
        return NSOF_OK;
    }
};

// Any early return of batch_host leaves copies in flight: uploads out of the caller's / the slots' pinned memory, downloads
// INTO the caller's flow arrays.  The caller is free to release those buffers as soon as it sees the error, so every
// non-OK exit drains the three streams first; the next call then finds idle slots.  Declared after everything a copy may
// still touch, so that it runs before any of that is destroyed.
struct Drain {
    nsof_ctx* ctx;
    nsof_pipe* pp;
    bool ok = false;
    ~Drain()
    {
        if (ok) return;
        (void)hipStreamSynchronize(pp->s_in);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(pp->s_out);
    }
};

// The pipelined host entry (pairs: HOST pointers; p.src gives the pixel size).
int batch_host(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc* pairs, const nsof_list_params& p)
{
    for (int i = 0; i < n_pairs; i++)
        if (int rc = nsof_farneback_list_check(ctx, i, pairs[i], p)) return rc;
    NSOF_HIP(ctx, hipSetDevice(ctx->device));
    nsof_pipe* pp;
    if (int rc = pipe_get(ctx, &pp)) return rc;
    g_pack_node = nsof_gpu_numa_node(ctx->device);
    PipeRun run(ctx, pp, n_pairs, pairs, p);
    Drain drain{ctx, pp};
    const int nc = (int)run.chunks.size();
    for (int ci = 0; ci < nc; ci++) {
        int rc;
        if ((rc = run.wait_for_slot(ci)) || (rc = run.reserve(ci))) return rc;
        run.pack(ci);
        if ((rc = run.upload(ci)) || (rc = run.compute(ci)) || (rc = run.download(ci))) return rc;
    }
    for (int ci = 0; ci < nc; ci++)
        if (!run.unpacked[ci])
            if (int rc = run.unpack(ci)) return rc;
    if (int rcs = nsof_stream_sync_checked(ctx)) return rcs;   // incl. a lost hand-over of the exact-order flow kernels
    run.trace.print(run.chunks);
    drain.ok = true;
    return NSOF_OK;
}

}  // namespace

extern "C" int nsof_farneback_px_batch(nsof_ctx* ctx, int pixel_type, int n_pairs, const nsof_pair_desc_px* pairs,
                                       double pyr_scale, int levels, int winsize, int iterations, int poly_n, double poly_sigma,
                                       int flags)
{
    if (int rc = nsof_check_typed(ctx, pixel_type)) return rc;
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return nsof_set_error(ctx, NSOF_EINVAL, "bad pair list");
    if (n_pairs == 0) return NSOF_OK;
    const nsof_list_params p(pixel_type, {pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags});
    return batch_host(ctx, n_pairs, reinterpret_cast<const nsof_pair_desc*>(pairs), p);
}

// ---- the 8-bit and float32 exports of this route: the typed entry with the pixel type named -----------------------------
extern "C" int nsof_farneback_u8_batch(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc* pairs, double pyr_scale,
                                       int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags)
{
    return nsof_farneback_px_batch(ctx, NSOF_PIXEL_U8, n_pairs, as_px(pairs), pyr_scale, levels, winsize, iterations, poly_n,
                                   poly_sigma, flags);
}

extern "C" int nsof_farneback_f32_batch(nsof_ctx* ctx, int n_pairs, const nsof_pair_desc_f32* pairs, double pyr_scale,
                                        int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags)
{
    return nsof_farneback_px_batch(ctx, NSOF_PIXEL_F32, n_pairs, as_px(pairs), pyr_scale, levels, winsize, iterations, poly_n,
                                   poly_sigma, flags);
}
