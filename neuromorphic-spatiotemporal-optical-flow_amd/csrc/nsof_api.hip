// libnsof.so host side: context, error channel, page-locked host memory, profiling hooks, filter taps, level geometry,
// stage entry points.
// (The Farneback level driver is farneback_driver.hip.)
#include <cctype>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <algorithm>
#include <cstring>

#include <sys/syscall.h>
#include <unistd.h>

#include "nsof_internal.h"

static char g_create_err[512] = "";

int nsof_set_error(nsof_ctx* ctx, int code, const char* fmt, ...)
{
    char* dst = ctx ? ctx->err : g_create_err;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dst, 512, fmt, ap);
    va_end(ap);
    return code;
}

int nsof_xsync_reserve(nsof_ctx* ctx, size_t carry_bytes, unsigned long long** carry, unsigned** tickets, unsigned** err)
{
    if (!ctx->x_sync.p) {
        if (int rc = ctx->x_sync.reserve(ctx, 2048)) return rc;
        NSOF_HIP(ctx, hipMemsetAsync(ctx->x_sync.p, 0, 2048, ctx->stream));
    }
    if (carry_bytes > ctx->x_carry.cap) {
        // some slack: shapes vary from call to call
        if (int rc = ctx->x_carry.reserve(ctx, carry_bytes, (carry_bytes + (carry_bytes >> 3) + 4095) & ~(size_t)4095)) return rc;
        NSOF_HIP(ctx, hipMemsetAsync(ctx->x_carry.p, 0, ctx->x_carry.cap, ctx->stream));   // tag 0 = never written
    }
    *carry = ctx->x_carry.p;
    *tickets = ctx->x_sync.p;
    *err = ctx->x_sync.p + 256;
    ctx->x_dirty = true;
    return NSOF_OK;
}

int nsof_xsync_check(nsof_ctx* ctx)
{
    if (!ctx->x_dirty || !ctx->x_sync.p) return NSOF_OK;
    ctx->x_dirty = false;
    unsigned w = 0;
    NSOF_HIP(ctx, hipMemcpy(&w, ctx->x_sync.p + 256, sizeof(w), hipMemcpyDeviceToHost));
    if (w) {
        NSOF_HIP(ctx, hipMemset(ctx->x_sync.p + 256, 0, sizeof(w)));
        return nsof_set_error(ctx, NSOF_EDEVICE, "exact-order iteration: a hand-over between workgroups / waves never arrived (flags %u); results are invalid", w);
    }
    return NSOF_OK;
}

int nsof_stream_sync_checked(nsof_ctx* ctx)
{
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return nsof_xsync_check(ctx);
}

// ---- profiling ---------------------------------------------------------------------------
nsof_prof_scope::nsof_prof_scope(nsof_ctx* c, int k) : ctx(c), id(k), on((c->prof_mask >> k) & 1u)
{
    if (!on) return;
    nsof_prof_slot& s = ctx->prof[id];
    if (s.used == s.start.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
        s.start.push_back(a);
        s.stop.push_back(b);
    }
    hipEventRecord(s.start[s.used], ctx->stream);
}
nsof_prof_scope::~nsof_prof_scope()
{
    if (!on) return;
    nsof_prof_slot& s = ctx->prof[id];
    hipEventRecord(s.stop[s.used], ctx->stream);
    s.used++;
}

extern "C" int nsof_prof_enable(nsof_ctx* ctx, unsigned mask)
{
    if (!ctx) return NSOF_EINVAL;
    ctx->prof_mask = mask & ((1u << NSOF_K_COUNT) - 1);
    return NSOF_OK;
}

extern "C" int nsof_prof_collect(nsof_ctx* ctx, int id, double* total_ms, long long* launches)
{
    if (!ctx || id < 0 || id >= NSOF_K_COUNT) return NSOF_EINVAL;
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->side) NSOF_HIP(ctx, hipStreamSynchronize(ctx->side));
    nsof_prof_slot& s = ctx->prof[id];
    for (size_t i = 0; i < s.used; i++) {
        float ms = 0;
        NSOF_HIP(ctx, hipEventElapsedTime(&ms, s.start[i], s.stop[i]));
        s.acc_ms += ms;
        s.acc_launches++;
    }
    s.used = 0;
    if (total_ms) *total_ms = s.acc_ms;
    if (launches) *launches = s.acc_launches;
    s.acc_ms = 0;
    s.acc_launches = 0;
    return NSOF_OK;
}

// ---- page-locked host memory next to the GPU ------------------------------------------------------------------
// On a two-socket host a pinned buffer on the far socket halves the PCIe copy rate (measured on the MI355X boxes:
// 28 instead of 57 GB/s).  The GPU's NUMA node comes from sysfs (PCI bus id -> numa_node); the allocation runs under
// a temporary MPOL_PREFERRED policy for that node (hipHostMallocNumaUser makes the runtime honour it).  Every step
// is best effort: without sysfs / the syscall the default placement is used.
int nsof_gpu_numa_node(int device)
{
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    for (char* c = bus; *c; c++) *c = (char)tolower(*c);
    char path[160];
    snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE* f = fopen(path, "r");
    if (!f) return -1;
    int node = -1;
    if (fscanf(f, "%d", &node) != 1) node = -1;
    fclose(f);
    return node;
}

void* nsof_pinned_alloc(int device, size_t bytes)
{
    void* p = nullptr;
    const int node = nsof_gpu_numa_node(device);
    bool policy = false;
    // the calling thread's own policy (an application may run under numactl --membind / --interleave): saved and restored
    int old_mode = 0;
    unsigned long old_mask[16] = {0};
    const bool have_old = syscall(SYS_get_mempolicy, &old_mode, old_mask, 8 * sizeof(old_mask) + 1, nullptr, 0) == 0;
    if (node >= 0 && node < 1024 && have_old) {
        unsigned long mask[16] = {0};
        mask[node / (8 * sizeof(unsigned long))] = 1ul << (node % (8 * sizeof(unsigned long)));
        policy = syscall(SYS_set_mempolicy, 1 /* MPOL_PREFERRED */, mask, 8 * sizeof(mask) + 1) == 0;
    }
    hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, policy ? hipHostMallocNumaUser : hipHostMallocDefault);
    if (policy) (void)syscall(SYS_set_mempolicy, old_mode, old_mode == 0 ? nullptr : old_mask, old_mode == 0 ? 0 : 8 * sizeof(old_mask) + 1);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}

extern "C" void* nsof_host_alloc(size_t bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = 0;
    }
    return nsof_pinned_alloc(dev, bytes);   // on the current device's NUMA node where the host lets us choose
}

extern "C" void nsof_host_free(void* p)
{
    if (p) (void)hipHostFree(p);
}

int nsof_buf_grow(nsof_ctx* ctx, bool pinned, void** p, size_t* cap, size_t need, size_t new_cap)
{
    if (*cap >= need) return NSOF_OK;
    if (*p) {
        NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));   // queued work may still touch the old allocation
        NSOF_HIP(ctx, pinned ? hipHostFree(*p) : hipFree(*p));
        *p = nullptr;
        *cap = 0;
    }
    if (pinned) {
        *p = nsof_pinned_alloc(ctx->device, new_cap);
        if (!*p) return nsof_set_error(ctx, NSOF_ENOMEM, "hipHostMalloc(%zu) failed", new_cap);
    } else if (hipError_t e = hipMalloc(p, new_cap)) {
        *p = nullptr;
        return nsof_set_error(ctx, NSOF_ENOMEM, "hipMalloc(%zu) failed: %s", new_cap, hipGetErrorString(e));
    }
    *cap = new_cap;
    return NSOF_OK;
}

int nsof_table::stage(nsof_ctx* ctx, size_t bytes, size_t cap)
{
    if (!ev) NSOF_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    else NSOF_HIP(ctx, hipEventSynchronize(ev));   // the previous upload has left the pinned copy
    if (int rc = h.reserve(ctx, bytes, cap)) return rc;
    return d.reserve(ctx, bytes, cap);
}

const void* nsof_table::upload(nsof_ctx* ctx, size_t bytes)
{
    hipError_t e = hipMemcpyAsync(d.p, h.p, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipEventRecord(ev, ctx->stream);
    if (e != hipSuccess) {
        nsof_set_error(ctx, NSOF_EDEVICE, "table upload (%zu bytes) failed: %s", bytes, hipGetErrorString(e));
        return nullptr;
    }
    return d.p;
}

extern "C" const char* nsof_kernel_name(int id)
{
    static const char* names[NSOF_K_COUNT] = {"prep", "polyexp", "flow_upsample", "update_matrices", "blur_solve",
                                              "accum_update", "iterate", "mask_pack", "morph_chain", "remap", "ssim"};
    return (id >= 0 && id < NSOF_K_COUNT) ? names[id] : "?";
}

// ---- context -----------------------------------------------------------------------------
extern "C" int nsof_abi_version(void) { return NSOF_ABI_VERSION; }

extern "C" int nsof_create(int device, nsof_ctx** out)
{
    if (!out) return NSOF_EINVAL;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return nsof_set_error(nullptr, NSOF_EDEVICE, "no HIP device available (%s); libnsof has no CPU fallback",
                              e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= count)
        return nsof_set_error(nullptr, NSOF_EINVAL, "device %d out of range (0..%d)", device, count - 1);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device)) != hipSuccess)
        return nsof_set_error(nullptr, NSOF_EDEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return nsof_set_error(nullptr, NSOF_EDEVICE, "device %d is %s; libnsof is built for gfx950 only", device,
                              prop.gcnArchName);
    if ((e = hipSetDevice(device)) != hipSuccess)
        return nsof_set_error(nullptr, NSOF_EDEVICE, "hipSetDevice: %s", hipGetErrorString(e));
    nsof_ctx* ctx = new (std::nothrow) nsof_ctx();
    if (!ctx) return nsof_set_error(nullptr, NSOF_ENOMEM, "out of host memory");
    ctx->device = device;
    if ((e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking)) != hipSuccess) {
        delete ctx;
        return nsof_set_error(nullptr, NSOF_EDEVICE, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    ctx->stream = ctx->own_stream;
    if (const char* e = getenv("NSOF_POLYEXP_F32")) ctx->opt_polyexp_f32 = (e[0] && e[0] != '0') ? 1 : 0;
    if (const char* e = getenv("NSOF_EXACT_ROWSUMS")) ctx->opt_exact_rowsums = (e[0] && e[0] != '0') ? 1 : 0;
    if (const char* e = getenv("NSOF_PYR_FMA")) ctx->opt_pyr_fma = (e[0] && e[0] != '0') ? 1 : 0;
    if (const char* e = getenv("NSOF_LAT_JOBS")) ctx->opt_small_batch_jobs = atoi(e) < 0 ? 0 : atoi(e);
    if (const char* e = getenv("NSOF_ROW_BANDS")) {
        const int v = atoi(e);
        ctx->opt_row_bands = v < 0 || v == 2 || v == 3 ? 0 : v;
    }
    *out = ctx;
    return NSOF_OK;
}

extern "C" void nsof_destroy(nsof_ctx* ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (auto& s : ctx->prof) {
        for (auto ev : s.start) hipEventDestroy(ev);
        for (auto ev : s.stop) hipEventDestroy(ev);
    }
    nsof_pipe_destroy(ctx);
    for (auto ev : ctx->ov_events) hipEventDestroy(ev);
    if (ctx->side) hipStreamDestroy(ctx->side);
    if (ctx->own_stream) hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" const char* nsof_last_error(const nsof_ctx* ctx) { return ctx ? ctx->err : g_create_err; }

extern "C" int nsof_set_stream(nsof_ctx* ctx, void* s)
{
    if (!ctx) return NSOF_EINVAL;
    NSOF_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = s ? (hipStream_t)s : ctx->own_stream;
    return NSOF_OK;
}

extern "C" int nsof_set_option(nsof_ctx* ctx, int option, int value)
{
    if (!ctx) return NSOF_EINVAL;
    if (option == NSOF_OPT_POLYEXP_F32 || option == NSOF_OPT_EXACT_ROWSUMS || option == NSOF_OPT_PYR_FMA) {
        if (value != 0 && value != 1) return nsof_set_error(ctx, NSOF_EINVAL, "option %d takes 0 or 1", option);
        (option == NSOF_OPT_POLYEXP_F32 ? ctx->opt_polyexp_f32 : option == NSOF_OPT_PYR_FMA ? ctx->opt_pyr_fma : ctx->opt_exact_rowsums) = value;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_ROW_BANDS) {
        if (value < 0 || value == 2 || value == 3)
            return nsof_set_error(ctx, NSOF_EINVAL, "NSOF_OPT_ROW_BANDS: 0 (off), 1 (automatic) or a row count >= 4");
        ctx->opt_row_bands = value;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_SMALL_BATCH_JOBS) {
        if (value < 0) return nsof_set_error(ctx, NSOF_EINVAL, "NSOF_OPT_SMALL_BATCH_JOBS: a job count >= 0");
        ctx->opt_small_batch_jobs = value;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_DEBUG_FAULT) {
        if (value < 0 || value > 3) return nsof_set_error(ctx, NSOF_EINVAL, "NSOF_OPT_DEBUG_FAULT: bits 0..1");
        ctx->dbg_fault = value;
        return NSOF_OK;
    }
    return nsof_set_error(ctx, NSOF_EINVAL, "unknown option %d", option);
}

extern "C" int nsof_get_option(const nsof_ctx* ctx, int option, int* value)
{
    if (!ctx || !value) return NSOF_EINVAL;
    if (option == NSOF_OPT_POLYEXP_F32) {
        *value = ctx->opt_polyexp_f32;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_EXACT_ROWSUMS) {
        *value = ctx->opt_exact_rowsums;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_ROW_BANDS) {
        *value = ctx->opt_row_bands;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_PYR_FMA) {
        *value = ctx->opt_pyr_fma;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_SMALL_BATCH_JOBS) {
        *value = ctx->opt_small_batch_jobs;
        return NSOF_OK;
    }
    if (option == NSOF_OPT_DEBUG_FAULT) {
        *value = ctx->dbg_fault;
        return NSOF_OK;
    }
    return NSOF_EINVAL;
}

extern "C" int nsof_synchronize(nsof_ctx* ctx)
{
    if (!ctx) return NSOF_EINVAL;
    return nsof_stream_sync_checked(ctx);
}

// ---- filter taps (host, double precision as the reference library computes them) -----------
static int round_half_even(double v) { return (int)lrint(v); }

int nsof_host_blur_taps(int ksize, double sigma, nsof_blur_taps* out)
{
    if (ksize < 1 || (ksize & 1) == 0 || ksize > NSOF_MAX_BLUR_TAPS - 1) return NSOF_EUNSUPPORTED;
    out->ksize = ksize;
    memset(out->k, 0, sizeof(out->k));
    if (sigma <= 0 && ksize <= 9) {  // fixed small tables
        static const double t1[] = {1.};
        static const double t3[] = {0.25, 0.5, 0.25};
        static const double t5[] = {0.0625, 0.25, 0.375, 0.25, 0.0625};
        static const double t7[] = {0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125};
        static const double t9[] = {4. / 256, 13. / 256, 30. / 256, 51. / 256, 60. / 256, 51. / 256, 30. / 256, 13. / 256, 4. / 256};
        const double* t = ksize == 1 ? t1 : ksize == 3 ? t3 : ksize == 5 ? t5 : ksize == 7 ? t7 : t9;
        for (int i = 0; i < ksize; i++) out->k[i] = (float)t[i];
        return NSOF_OK;
    }
    const double sg = sigma > 0 ? sigma : ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2 = -0.125 / (sg * sg);
    const int h = (ksize - 1) / 2;
    double v[NSOF_MAX_BLUR_TAPS], sum = 0;
    for (int i = 0, x = 1 - ksize; i < h; i++, x += 2) {
        v[i] = std::exp((double)(x * x) * scale2);
        sum += v[i];
    }
    sum = sum * 2.0 + 1.0;
    const double inv = 1.0 / sum;
    for (int i = 0; i < h; i++) out->k[i] = out->k[ksize - 1 - i] = (float)(v[i] * inv);
    out->k[h] = (float)inv;
    return NSOF_OK;
}

static bool chol_inv6(const double A[6][6], double inv[6][6])
{
    double L[6][6] = {{0}};
    for (int i = 0; i < 6; i++)
        for (int j = 0; j <= i; j++) {
            double s = A[i][j];
            for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (s <= 0) return false;
                L[i][i] = std::sqrt(s);
            } else
                L[i][j] = s / L[j][j];
        }
    for (int c = 0; c < 6; c++) {
        double y[6], x[6];
        for (int i = 0; i < 6; i++) {
            double s = (i == c) ? 1. : 0.;
            for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
            y[i] = s / L[i][i];
        }
        for (int i = 5; i >= 0; i--) {
            double s = y[i];
            for (int k = i + 1; k < 6; k++) s -= L[k][i] * x[k];
            x[i] = s / L[i][i];
        }
        for (int i = 0; i < 6; i++) inv[i][c] = x[i];
    }
    return true;
}

int nsof_host_poly_taps(int n, double sigma, nsof_poly_taps* out)
{
    if (n < 1 || n > NSOF_MAX_POLY_N) return NSOF_EUNSUPPORTED;
    if (sigma < FLT_EPSILON) sigma = n * 0.3;
    float g[2 * NSOF_MAX_POLY_N + 1], xg[2 * NSOF_MAX_POLY_N + 1], xxg[2 * NSOF_MAX_POLY_N + 1];
    double s = 0.;
    for (int x = -n; x <= n; x++) {
        g[x + n] = (float)std::exp(-x * x / (2 * sigma * sigma));
        s += g[x + n];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        g[x + n] = (float)(g[x + n] * s);
        xg[x + n] = (float)(x * g[x + n]);
        xxg[x + n] = (float)(x * x * g[x + n]);
    }
    double G[6][6] = {{0}}, inv[6][6];
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            G[0][0] += g[y + n] * g[x + n];
            G[1][1] += g[y + n] * g[x + n] * x * x;
            G[3][3] += g[y + n] * g[x + n] * x * x * x * x;
            G[5][5] += g[y + n] * g[x + n] * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    if (!chol_inv6(G, inv)) return NSOF_EINVAL;
    memset(out, 0, sizeof(*out));
    out->n = n;
    for (int k = 0; k <= n; k++) {
        out->g[k] = g[n + k];
        out->xg[k] = xg[n + k];
        out->xxg[k] = xxg[n + k];
        out->dg[k] = (double)g[n + k];
        out->dxxg[k] = (double)xxg[n + k];
    }
    out->ig11 = inv[1][1];
    out->ig03 = inv[0][3];
    out->ig33 = inv[3][3];
    out->ig55 = inv[5][5];
    return NSOF_OK;
}

// ---- level geometry ------------------------------------------------------------------------
extern "C" int nsof_farneback_effective_levels(int width, int height, double pyr_scale, int levels)
{
    int k;
    double scale = 1;
    for (k = 0; k < levels; k++) {
        scale *= pyr_scale;
        if (width * scale < 32 || height * scale < 32) break;
    }
    return k;
}

extern "C" int nsof_farneback_level_size(int width, int height, double pyr_scale, int level, int* lw, int* lh,
                                          int* ksize, double* sigma)
{
    if (width < 1 || height < 1 || level < 0 || !(pyr_scale > 0) || !(pyr_scale < 1)) return NSOF_EINVAL;
    double scale = 1;
    for (int i = 0; i < level; i++) scale *= pyr_scale;
    const double sg = (1. / scale - 1) * 0.5;
    int sz = round_half_even(sg * 5) | 1;
    if (sz < 3) sz = 3;
    if (lw) *lw = round_half_even(width * scale);
    if (lh) *lh = round_half_even(height * scale);
    if (ksize) *ksize = sz;
    if (sigma) *sigma = sg;
    return NSOF_OK;
}

int nsof_check_farneback_params(nsof_ctx* ctx, int width, int height, const nsof_fb_params& p)
{
    const int levels = p.levels, winsize = p.winsize, iterations = p.iterations, poly_n = p.poly_n, flags = p.flags;
    if (width < 1 || height < 1) return nsof_set_error(ctx, NSOF_ESHAPE, "empty image %dx%d", width, height);
    if ((long long)width * height > (1ll << 27))   // kernels address one image with 32-bit byte offsets
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "image %dx%d exceeds 2^27 pixels", width, height);
    if (!(p.pyr_scale > 0) || !(p.pyr_scale < 1))
        return nsof_set_error(ctx, NSOF_EINVAL, "pyr_scale=%g must be in (0,1)", p.pyr_scale);
    if (winsize == 1)  // upstream's running sums are ill-formed for a 1x1 window (m = 0); never used by the reference
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "winsize=1 is not supported");
    if (levels < 0 || winsize < 1 || iterations < 0)
        return nsof_set_error(ctx, NSOF_EINVAL, "levels=%d winsize=%d iterations=%d invalid", levels, winsize,
                              iterations);
    if (poly_n < 1 || poly_n > NSOF_MAX_POLY_N)
        return nsof_set_error(ctx, poly_n < 1 ? NSOF_EINVAL : NSOF_EUNSUPPORTED, "poly_n=%d outside 1..%d", poly_n,
                              NSOF_MAX_POLY_N);
    if (flags != 0 && flags != NSOF_FARNEBACK_GAUSSIAN)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED,
                              "flags=%d: OPTFLOW_USE_INITIAL_FLOW (4) is not implemented, and no bit other than 256 is known",
                              flags);
    if (flags && winsize / 2 > NSOF_GAUSS_MAX_M)
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "winsize=%d too large for the Gaussian window (max %d)", winsize,
                              2 * NSOF_GAUSS_MAX_M + 1);
    return NSOF_OK;
}

// ---- frame layout ---------------------------------------------------------------------------------------------------
// The layout rule of frames of pixel type src (nsof_src_type), stated once: p is one frame, or the first of a stack of
// frames img_stride bytes apart (0 for a lone frame).  Frames are addressed with byte strides whatever the pixel type, so
// every pixel must stay aligned to its size: the start address and both strides multiples of the pixel size, and a row
// stride that holds a row.  The kernels take their vector forms only where rows are aligned for them and scalar loads
// elsewhere, so crops that start at any element are fine.  1-byte pixels have nothing to check here: what the 8-bit
// routes ask of a row stride stays with their drivers.  `who` (printf-style) names the frame in the message.
int nsof_check_frame_layout(nsof_ctx* ctx, int src, const void* p, ptrdiff_t row_stride, ptrdiff_t img_stride, int width,
                            const char* who, ...)
{
    const ptrdiff_t px = nsof_src_bytes(src);
    if (px == 1 || (reinterpret_cast<uintptr_t>(p) % px == 0 && row_stride % px == 0 && img_stride % px == 0 &&
                    row_stride >= px * width))
        return NSOF_OK;
    char name[64];
    va_list ap;
    va_start(ap, who);
    vsnprintf(name, sizeof(name), who, ap);
    va_end(ap);
    return nsof_set_error(ctx, NSOF_EINVAL, "%s: %td-byte pixels need the address, the row stride (%td) and the image stride (%td) "
                          "to be multiples of %td and the row stride >= %td*width", name, px, row_stride, img_stride, px, px);
}

// ---- stage entry points ---------------------------------------------------------------------
extern "C" int nsof_stage_pyr_level_px(nsof_ctx* ctx, int pixel_type, int n_img, const void* d_src, ptrdiff_t row_stride,
                                       ptrdiff_t img_stride, int width, int height, double pyr_scale, int level, float* d_out)
{
    if (int rc = nsof_check_typed(ctx, pixel_type)) return rc;
    if (!d_src || !d_out || n_img < 1) return NSOF_EINVAL;
    if (int rc = nsof_check_frame_layout(ctx, pixel_type, d_src, row_stride, img_stride, width, "d_src")) return rc;
    int wk, hk;
    nsof_blur_taps taps;
    if (int rc = nsof_level_geom(ctx, width, height, pyr_scale, level, &wk, &hk, &taps)) return rc;
    return nsof_launch_prep(ctx, n_img, d_src, row_stride, img_stride, width, height, wk, hk, taps, d_out, pixel_type);
}

extern "C" int nsof_stage_pyr_level(nsof_ctx* ctx, int n_img, const uint8_t* d_src, ptrdiff_t row_stride,
                                    ptrdiff_t img_stride, int width, int height, double pyr_scale, int level,
                                    float* d_out)
{
    return nsof_stage_pyr_level_px(ctx, NSOF_PIXEL_U8, n_img, d_src, row_stride, img_stride, width, height, pyr_scale, level, d_out);
}

extern "C" int nsof_stage_pyr_level_f32(nsof_ctx* ctx, int n_img, const float* d_src, ptrdiff_t row_stride,
                                        ptrdiff_t img_stride, int width, int height, double pyr_scale, int level,
                                        float* d_out)
{
    return nsof_stage_pyr_level_px(ctx, NSOF_PIXEL_F32, n_img, d_src, row_stride, img_stride, width, height, pyr_scale, level, d_out);
}

__global__ void k_recip_probe(long long n, const double* __restrict__ x, double* __restrict__ fast, double* __restrict__ ieee)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        fast[i] = nsof_recip_normal(x[i]);
        ieee[i] = 1. / x[i];
    }
}

extern "C" int nsof_stage_recip(nsof_ctx* ctx, long long n, const double* d_x, double* d_out, double* d_ieee)
{
    if (!ctx || !d_x || !d_out || !d_ieee || n < 1) return NSOF_EINVAL;
    hipLaunchKernelGGL(k_recip_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, n, d_x, d_out, d_ieee);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}

extern "C" int nsof_stage_polyexp(nsof_ctx* ctx, int n_img, const float* d_img, int width, int height, int poly_n,
                                  double poly_sigma, float* d_R)
{
    if (!ctx || !d_img || !d_R || n_img < 1 || width < 1 || height < 1) return NSOF_EINVAL;
    nsof_poly_taps taps;
    int rc = nsof_host_poly_taps(poly_n, poly_sigma, &taps);
    if (rc) return nsof_set_error(ctx, rc, "poly_n=%d unsupported", poly_n);
    return nsof_launch_polyexp(ctx, n_img, d_img, width, height, taps, d_R);
}

extern "C" int nsof_stage_update_matrices(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_flow,
                                          int width, int height, float* d_M)
{
    if (!ctx || !d_R || !d_flow || !d_M || n_pairs < 1 || width < 1 || height < 1) return NSOF_EINVAL;
    const size_t plane = (size_t)width * height;
    return nsof_launch_update_matrices(ctx, n_pairs, d_R, d_R + 5 * plane, 10 * plane, d_flow, width, height, d_M);
}

extern "C" int nsof_stage_blur_solve(nsof_ctx* ctx, int n_pairs, const float* d_M, int width, int height,
                                     int winsize, float* d_flow)
{
    if (!ctx || !d_M || !d_flow || n_pairs < 1 || width < 1 || height < 1 || winsize < 2) return NSOF_EINVAL;
    // the library's row-sum order (k_blur_colsum + k_blur_rowsolve) wherever the driver's form is exact
    if (nsof_form_exact(nsof_iterate_form(ctx, winsize, width, height, 1, n_pairs * nsof_iterate_jobs(width, height), 0))) {
        const size_t need = (size_t)n_pairs * 5 * width * height * sizeof(double);
        if (int rc = ctx->ws.reserve(ctx, need)) return rc;
        return nsof_launch_blur_solve_exact(ctx, n_pairs, d_M, width, height, winsize, (double*)ctx->ws.p, d_flow);
    }
    return nsof_launch_blur_solve(ctx, n_pairs, d_M, width, height, winsize, d_flow);
}

extern "C" int nsof_stage_gauss_blur_solve(nsof_ctx* ctx, int n_pairs, const float* d_M, int width, int height,
                                           int winsize, float* d_flow)
{
    if (!ctx || !d_M || !d_flow || n_pairs < 1 || n_pairs > 65535 || width < 1 || height < 1 || winsize < 2) return NSOF_EINVAL;
    return nsof_launch_gauss_blur_solve(ctx, n_pairs, d_M, width, height, winsize, d_flow);
}

extern "C" int nsof_stage_iterate(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_flow_in, int width,
                                  int height, int winsize, float* d_flow_out)
{
    if (!ctx || !d_R || !d_flow_in || !d_flow_out || d_flow_in == d_flow_out || n_pairs < 1 || width < 1 || height < 1)
        return NSOF_EINVAL;
    const nsof_iter_form form = nsof_iterate_form(ctx, winsize, width, height, 1, n_pairs * nsof_iterate_jobs(width, height), 0);
    if (!nsof_form_fused(form)) return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "winsize %d not fused", winsize);
    const size_t plane = (size_t)width * height;
    if (form == NSOF_ITER_FAST)
        return nsof_launch_iterate(ctx, n_pairs, d_R, d_R + 5 * plane, 10 * plane, d_flow_in, d_flow_out, width, height,
                                   winsize);
    // the exact order in its one-kernel form, small batches too (the stage has no workspace for the small-batch form)
    return nsof_launch_iterate_x(ctx, n_pairs, d_R, d_R + 5 * plane, 10 * plane, d_flow_in, d_flow_out, width, height,
                                 winsize);
}

extern "C" int nsof_stage_iterate_upsample(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_coarse_flow,
                                           int src_w, int src_h, int width, int height, int winsize, double pyr_scale,
                                           float* d_flow_out)
{
    if (!ctx || !d_R || !d_coarse_flow || !d_flow_out || n_pairs < 1 || width < 1 || height < 1 || src_w < 1 || src_h < 1)
        return NSOF_EINVAL;
    (void)pyr_scale;
    return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "fused upsample+iteration not available for winsize %d", winsize);
}

extern "C" int nsof_stage_iterate_x_resample(nsof_ctx* ctx, int n_pairs, const float* d_R, const float* d_coarse_flow,
                                             int src_w, int src_h, int width, int height, int winsize, double pyr_scale,
                                             float* d_flow_out)
{
    if (!ctx || !d_R || !d_coarse_flow || !d_flow_out || d_coarse_flow == d_flow_out || n_pairs < 1 || width < 1 || height < 1 ||
        src_w < 1 || src_h < 1)
        return NSOF_EINVAL;
    const size_t plane = (size_t)width * height;
    return nsof_launch_iterate_x_resample(ctx, n_pairs, d_R, d_R + 5 * plane, 10 * plane, d_coarse_flow, src_w, src_h,
                                          (float)(1. / pyr_scale), d_flow_out, width, height, winsize);
}

extern "C" int nsof_stage_flow_upsample(nsof_ctx* ctx, int n_pairs, const float* d_src, int sw, int sh, float* d_dst,
                                        int dw, int dh, double pyr_scale)
{
    if (!ctx || !d_src || !d_dst || n_pairs < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return NSOF_EINVAL;
    return nsof_launch_flow_upsample(ctx, n_pairs, d_src, sw, sh, d_dst, dw, dh, (float)(1. / pyr_scale));
}

// ---- ROI gating (host arithmetic on maps of at most a few hundred cells) -------------------------------------------
extern "C" int nsof_roi_from_surface(const double* current, int rows, int cols, int frame_w, int frame_h, int memsize,
                                     int thres, int extend_left, int extend_right, int extend_upper, int extend_lower,
                                     int connectivity, int flag, int* rects, int max_rects)
{
    if (!current || rows < 1 || cols < 1 || frame_w < 1 || frame_h < 1 || memsize < 1 || (connectivity != 4 && connectivity != 8) ||
        (flag != 1 && flag != 2) || max_rects < 0 || (max_rects > 0 && !rects))
        return NSOF_EINVAL;
    const int th = frame_h / memsize, tw = frame_w / memsize;   // the transition picture: int(h / MS) x int(w / MS)
    if (rows > th || cols > tw) return NSOF_ESHAPE;             // the reference's numba loop would write out of bounds
    std::vector<int> lab((size_t)th * tw, 0);
    std::vector<unsigned char> on((size_t)th * tw, 0);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < cols; x++) {
            double g = -3366.0 / std::log10(current[(size_t)y * cols + x]) - 306.0;
            g = g < 0.0 ? 0.0 : (g > 255.0 ? 255.0 : g);        // NaN (I <= 0) compares false twice and casts to 0
            const int gi = (g == g) ? (int)(unsigned char)g : 0;
            on[(size_t)y * tw + x] = gi >= thres;
        }
    struct Box { int x0, y0, x1, y1; };
    std::vector<Box> boxes;
    std::vector<int> stack;
    for (int y = 0; y < th; y++)
        for (int x = 0; x < tw; x++) {
            if (!on[(size_t)y * tw + x] || lab[(size_t)y * tw + x]) continue;
            boxes.push_back({x, y, x, y});
            const int id = (int)boxes.size();
            lab[(size_t)y * tw + x] = id;
            stack.assign(1, y * tw + x);
            while (!stack.empty()) {
                const int p = stack.back();
                stack.pop_back();
                const int py = p / tw, px = p % tw;
                Box& b = boxes[id - 1];
                b.x0 = px < b.x0 ? px : b.x0; b.x1 = px > b.x1 ? px : b.x1;
                b.y0 = py < b.y0 ? py : b.y0; b.y1 = py > b.y1 ? py : b.y1;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        if ((!dx && !dy) || (connectivity == 4 && dx && dy)) continue;
                        const int ny = py + dy, nx = px + dx;
                        if (ny < 0 || ny >= th || nx < 0 || nx >= tw) continue;
                        const size_t q = (size_t)ny * tw + nx;
                        if (on[q] && !lab[q]) { lab[q] = id; stack.push_back((int)q); }
                    }
            }
        }
    if (boxes.empty()) return 0;
    if (flag == 2) {   // union box of all components
        Box u = boxes[0];
        for (const Box& b : boxes) {
            u.x0 = b.x0 < u.x0 ? b.x0 : u.x0; u.y0 = b.y0 < u.y0 ? b.y0 : u.y0;
            u.x1 = b.x1 > u.x1 ? b.x1 : u.x1; u.y1 = b.y1 > u.y1 ? b.y1 : u.y1;
        }
        boxes.assign(1, u);
    }
    int n = 0;
    for (const Box& b : boxes) {
        const int x0 = std::max(b.x0 * memsize - extend_left, 0), y0 = std::max(b.y0 * memsize - extend_upper, 0);
        const int x1 = std::min((b.x1 + 1) * memsize + extend_right, frame_w), y1 = std::min((b.y1 + 1) * memsize + extend_lower, frame_h);
        if (n < max_rects) { rects[4 * n] = x0; rects[4 * n + 1] = y0; rects[4 * n + 2] = x1; rects[4 * n + 3] = y1; }
        n++;
    }
    return n;
}
