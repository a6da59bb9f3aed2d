// Farneback dense optical flow, polynomial expansion (FarnebackPolyExp): k_polyexp_rs, the reference library's
// arithmetic, and the opt-in float kernel k_polyexp, for gfx950 (CDNA4, wave64).  Compiled with -ffp-contract=off: a*b+c
// stays two roundings unless fma() is written explicitly (DESIGN.md "numerics contract").
//
// HBM/L2-bound stencils: no MFMA.  Layouts: images [n][h][w] f32; R per image: [h][w][4] f32 (channels 0-3 interleaved:
// one 16-B access per pixel) followed by [h][w] f32 (channel 4) -- the L1 serves 4 lanes per cycle whatever the access
// width, so the gather of the matrix update wants few, wide loads.
#include <type_traits>

#include "nsof_internal.h"

namespace {

// ---------------------------------------------------------------------------------------
// Polynomial expansion (FarnebackPolyExp).  24 B/px algorithmic: 4 read + 5 x 4 written.
//
// "Strip walker": a block owns 256 image columns (SW output columns + NP halo on each side)
// and walks down a row segment four rows per step.
//   vertical pass   thread <-> column; the 2N+1 input rows of the column live in a register
//                   window (one coalesced dword load per thread per new row, prefetched one
//                   step ahead); r0/r1/r2 (float accumulation) go to LDS.
//   horizontal pass wave <-> row, lane <-> 4 adjacent pixels; taps come from LDS as
//                   ds_read_b128 and are reused across the 4 pixels in registers; in the exact
//                   kernel (k_polyexp_rs) the six moments accumulate in double exactly as the
//                   reference library does (b1,b4: double products -- exact, so written as fma;
//                   b2,b3,b5,b6: float products widened afterwards); 5 coalesced float4 stores
//                   per lane.
// ---------------------------------------------------------------------------------------
template <int N>
struct PolyGeom {
    static constexpr int NP = (N + 3) / 4 * 4;  // halo padded so LDS vectors stay 16-B aligned
    static constexpr int SW = 256 - 2 * NP;     // output columns per block
    static constexpr int NV = (2 * NP + 4) / 4; // float4 per lane per moment row
};

// The NSOF_OPT_POLYEXP_F32 kernel (opt-in, nsof_set_option): the horizontal moments accumulate in float (fma) instead
// of double -- NOT the reference library's arithmetic; results differ from the exact kernel (k_polyexp_rs) in the last
// bits of R (see DESIGN.md for the measured end-point error).  To keep the float sums small the image is taken relative
// to a per-workgroup constant c (a constant image has zero derivatives, so the outputs do not depend on c; the
// second-derivative outputs b1*ig03 + b5*ig33 cancel their two large terms, which is where float would lose most).
// `items` is unused: the argument list is the one k_polyexp_rs shares with its work-list form.
template <int N>
__global__ __launch_bounds__(256) void k_polyexp(const float* __restrict__ img, float* __restrict__ R, int W, int H,
                                                  int seg_rows, nsof_poly_taps tp,
                                                  const nsof_het_item* __restrict__ items)
{
    using G = PolyGeom<N>;
    const size_t img_off = (size_t)blockIdx.z * W * H;   // element offsets of this image / its expansion
    const size_t r_off = (size_t)blockIdx.z * 5 * W * H;
    __shared__ __attribute__((aligned(16))) float sr[2][3][4][256];
    __shared__ float ftap[2][N + 1];   // g, xg for the horizontal pass when N is large (see below)
    __shared__ float4 st[4][256];   // per-wave transpose buffer for the interleaved channel-0..3 stores

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid <= N) {
        ftap[0][tid] = tp.g[tid];
        ftap[1][tid] = tp.xg[tid];
    }
    const int x0 = blockIdx.x * G::SW;
    const int ys = blockIdx.y * seg_rows, ye = min(ys + seg_rows, H);
    const unsigned plane = (unsigned)W * (unsigned)H;
    // wave-uniform bases + 32-bit byte offsets: loads/stores stay in "SGPR base + VGPR offset" form
    const char* Ib = reinterpret_cast<const char*>(img + img_off);
    char* Rb = reinterpret_cast<char*>(R + r_off);
    const int xc = clampi(x0 - G::NP + tid, 0, W - 1);
    auto ld = [&](int row) {
        return *reinterpret_cast<const float*>(Ib + ((unsigned)clampi(row, 0, H - 1) * (unsigned)W + (unsigned)xc) * 4u);
    };

    // everything relative to the workgroup's first pixel
    const float cref = *reinterpret_cast<const float*>(Ib + ((unsigned)clampi(ys, 0, H - 1) * (unsigned)W + (unsigned)clampi(x0, 0, W - 1)) * 4u);
    // register window: win[j] = I[clamp(y - N + j)][xc]
    float win[2 * N + 1];
#pragma unroll
    for (int j = 0; j <= 2 * N; j++) win[j] = ld(ys - N + j) - cref;
    float pre[4];
#pragma unroll
    for (int q = 0; q < 4; q++) pre[q] = ld(ys + 1 + N + q) - cref;

    int buf = 0;
    for (int y = ys; y < ye; y += 4, buf ^= 1) {
        float nxt[4];
#pragma unroll
        for (int q = 0; q < 4; q++) nxt[q] = ld(y + 5 + N + q) - cref;

        // ---- vertical pass: 4 rows for this thread's column
#pragma unroll
        for (int q = 0; q < 4; q++) {
            float t0 = win[N] * tp.g[0], t1 = 0.f, t2 = 0.f;
#pragma unroll
            for (int k = 1; k <= N; k++) {
                const float a = win[N - k], b = win[N + k];
                const float p = a + b;
                t0 = fmaf(tp.g[k], p, t0);
                t2 = fmaf(tp.xxg[k], p, t2);
                t1 = fmaf(tp.xg[k], b - a, t1);
            }
            sr[buf][0][q][tid] = t0;
            sr[buf][1][q][tid] = t1;
            sr[buf][2][q][tid] = t2;
#pragma unroll
            for (int j = 0; j < 2 * N; j++) win[j] = win[j + 1];
            win[2 * N] = pre[q];
        }
#pragma unroll
        for (int q = 0; q < 4; q++) pre[q] = nxt[q];
        __syncthreads();

        // ---- horizontal pass: wave <-> row, lane <-> 4 pixels; each moment row is consumed and its
        //      outputs stored before the next one is read (keeps the live register set small)
        const int yo = y + wave;
        const int xo = x0 + 4 * lane;
        if (4 * lane < G::SW && yo < ye && xo < W) {
            const unsigned opix = (unsigned)yo * (unsigned)W + (unsigned)xo;
            auto load_row = [&](int a, float (&v)[4 * G::NV]) {
                const float4* p4 = reinterpret_cast<const float4*>(&sr[buf][a][wave][4 * lane]);
#pragma unroll
                for (int i = 0; i < G::NV; i++) {
                    const float4 f = p4[i];
                    v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
                }
            };
            float o0[4], o1[4], o2[4], o3[4], o4[4];
            // float accumulation, taps in registers (xxg included), one moment row at a time.  Large radii: the
            // float taps would not fit the scalar register file (the spills cost more than the arithmetic), so g and
            // xg come from LDS into VGPRs.
            float fg[N + 1], fxg[N + 1], fxxg[N + 1];
#pragma unroll
            for (int k = 0; k <= N; k++) {
                fg[k] = (N > 7) ? ftap[0][k] : tp.g[k];
                fxg[k] = (N > 7) ? ftap[1][k] : tp.xg[k];
                fxxg[k] = tp.xxg[k];
            }
            const float i11 = (float)tp.ig11, i03 = (float)tp.ig03, i33 = (float)tp.ig33, i55 = (float)tp.ig55;
            float t03f[4];   // b1 * ig03, shared by the xx and yy outputs
            {
                float v[4 * G::NV];
                load_row(0, v);
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int c = G::NP + p;
                    float a1 = v[c] * fg[0], a2 = 0.f, a4 = 0.f;
#pragma unroll
                    for (int k = 1; k <= N; k++) {
                        const float hi = v[c + k], lo = v[c - k], sm = hi + lo;
                        a1 = fmaf(sm, fg[k], a1);
                        a4 = fmaf(sm, fxxg[k], a4);
                        a2 = fmaf(hi - lo, fxg[k], a2);
                    }
                    t03f[p] = a1 * i03;
                    o1[p] = a2 * i11;
                    o3[p] = fmaf(a4, i33, t03f[p]);
                }
            }
            {
                float v[4 * G::NV];
                load_row(1, v);
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int c = G::NP + p;
                    float a3 = v[c] * fg[0], a6 = 0.f;
#pragma unroll
                    for (int k = 1; k <= N; k++) {
                        const float hi = v[c + k], lo = v[c - k];
                        a3 = fmaf(hi + lo, fg[k], a3);
                        a6 = fmaf(hi - lo, fxg[k], a6);
                    }
                    o0[p] = a3 * i11;
                    o4[p] = a6 * i55;
                }
            }
            {
                float v[4 * G::NV];
                load_row(2, v);
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const int c = G::NP + p;
                    float a5 = v[c] * fg[0];
#pragma unroll
                    for (int k = 1; k <= N; k++) a5 = fmaf(v[c + k] + v[c - k], fg[k], a5);
                    o2[p] = fmaf(a5, i33, t03f[p]);
                }
            }
            // channel 4 of the lane's 4 pixels: one 16-B store
            float* c4 = reinterpret_cast<float*>(Rb) + 4u * plane + opix;
            if ((W & 3) == 0) {
                nsof_store_stream4(c4, o4[0], o4[1], o4[2], o4[3]);
            } else {
#pragma unroll
                for (int p = 0; p < 4; p++)
                    if (xo + p < W) c4[p] = o4[p];
            }
            // channels 0-3: a lane holds 4 consecutive pixels x 16 B; stored as is, one instruction would write 16 B
            // per lane at a 64-B stride.  Transpose through LDS (per wave) so that every store instruction writes
            // 64 consecutive pixels = 1 KiB contiguous.
#pragma unroll
            // (swizzled within each lane's 4 slots: unswizzled, the 8 lanes a ds_write_b128 serves per LDS cycle hit
            //  only 2 of the 8 bank groups -- PMC: 63 % of this kernel's LDS cycles were bank conflicts)
            for (int p = 0; p < 4; p++) st[wave][4 * lane + (p ^ ((lane >> 1) & 3))] = make_float4(o0[p], o1[p], o2[p], o3[p]);
        }
        {
            // every lane of the wave takes part (lanes beyond the strip read slots nobody wrote, and do not store)
            const int yo2 = y + wave;
            float4* q4 = reinterpret_cast<float4*>(Rb) + (unsigned)yo2 * (unsigned)W + (unsigned)x0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int px = 64 * k + lane;   // pixel within the strip row
                const float4 v = st[wave][(px & ~3) | ((px & 3) ^ ((px >> 3) & 3))];   // pixel px sits in lane px/4's slot
                if (px < G::SW && yo2 < ye && x0 + px < W) nsof_store_stream4(reinterpret_cast<float*>(q4 + px), v.x, v.y, v.z, v.w);
            }
        }
        // no second barrier: the next step writes the other LDS buffer (st is private to a wave)
    }
}

// ---------------------------------------------------------------------------------------
// Role-specialised strip walker (the default, the reference library's arithmetic): the same two passes as k_polyexp,
// run by different waves.  A workgroup has 8 waves: waves 0-3 (thread <-> column) run the vertical pass
// of step t+1 while waves 4-7 (wave <-> row, lane <-> 4 pixels) run the horizontal pass of step t on the other half of
// the double-buffered moment rows; one barrier per step.  Neither role carries the other's registers across its
// pass (the column window of 2N+1 rows on one side, the moment window and the double taps on the other), so the
// taps stay in scalar registers and radius 10 fits 4 waves per SIMD where the single-role kernel spilled at 256.
// Occupancy: 40 KiB of LDS lets 4 workgroups (8 waves per SIMD) share a CU when a wave fits 64 VGPRs and 80 SGPRs.  The
// horizontal pass hands each output on as soon as it is final (moment row 2 before row 1, so b1 * ig03 dies early), which
// keeps it near 46 VGPRs at N = 5 (82 when o0..o4 and t03 lived across all three rows: 2 workgroups per CU); for N <= 7
// the launch bound asks for the 80 SGPRs, paid with a few scalar taps kept in VGPR lanes (v_readlane in the loop).
// tests/test_codeobj_polyexp_budget.py holds the code object to that budget.
// ---------------------------------------------------------------------------------------
// FRAME (the full-resolution level): the level image is not read from memory but formed in the vertical pass from the
// integer frame itself (SRC: uint8_t, uint16_t or int16_t pixels) -- the 3 x 3 [k1 k0 k1] smoothing of k_prep_same3_vec,
// operation for operation -- so the pyramid kernel of level 0 and the 8 B/px its image costs (written there, read here)
// disappear; the vertical-pass waves have the issue slots for it (187 of their step's ~500 instruction slots were used).
struct PolyFrame {
    const uint8_t* src0;   // images [0, nsplit) at src0 + z * img_stride, the others at src1 + (z - nsplit) * img_stride
    const uint8_t* src1;   // (byte addresses)
    long long row_stride, img_stride;
    int nsplit;
    float k0, k1;          // centre and side tap
};
template <int N, bool HET, bool FRAME = false, typename SRC = uint8_t>
__global__ __launch_bounds__(512, N <= 7 ? 8 : 1) void k_polyexp_rs(const float* __restrict__ img, float* __restrict__ R, int W, int H,
                                                     int seg_rows, nsof_poly_taps tp,
                                                     const nsof_het_item* __restrict__ items, PolyFrame fr = PolyFrame{})
{
    using G = PolyGeom<N>;
    size_t img_off, r_off;   // element offsets of this image / its expansion
    const uint8_t* sb = nullptr;   // FRAME: this image's frame (byte address)
    long long srs = 0;
    if constexpr (HET) {
        const nsof_het_item& it = items[blockIdx.z >> 1];
        const size_t which = blockIdx.z & 1;
        W = it.wk;
        H = it.hk;
        if (blockIdx.x * G::SW >= W || blockIdx.y * seg_rows >= H) return;   // block-uniform, before any barrier
        img_off = it.offI + which * (size_t)W * H;
        r_off = it.offR + which * 5 * (size_t)W * H;
        if constexpr (FRAME) {
            sb = it.src[which];
            srs = it.src_stride[which];
        }
    } else {
        img_off = (size_t)blockIdx.z * W * H;
        r_off = (size_t)blockIdx.z * 5 * W * H;
        if constexpr (FRAME) {
            const int z = blockIdx.z;
            sb = z < fr.nsplit ? fr.src0 + (ptrdiff_t)z * fr.img_stride : fr.src1 + (ptrdiff_t)(z - fr.nsplit) * fr.img_stride;
            srs = fr.row_stride;
        }
    }
    __shared__ __attribute__((aligned(16))) float sr[2][3][4][256];
    // per-wave transpose buffer for the interleaved channel-0..3 stores, one plane per channel: st[wave][c][pixel]
    __shared__ __attribute__((aligned(16))) float st[4][4][256];

    const int tid = threadIdx.x & 255, lane = tid & 63, wave = tid >> 6;   // within the role
    const int role = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    const int x0 = blockIdx.x * G::SW;
    const int ys = blockIdx.y * seg_rows, ye = min(ys + seg_rows, H);
    const int nsteps = (ye - ys + 3) / 4;
    const unsigned plane = (unsigned)W * (unsigned)H;

    if (role == 0) {
        // ---- vertical pass: 4 rows per step for this thread's column
        const char* Ib = reinterpret_cast<const char*>(img + img_off);
        const int xc = clampi(x0 - G::NP + tid, 0, W - 1);
        auto ld = [&](int row) {
            return *reinterpret_cast<const float*>(Ib + ((unsigned)clampi(row, 0, H - 1) * (unsigned)W + (unsigned)xc) * 4u);
        };
        // FRAME: I[rc][xc] from the frame.  The rows are asked for in order, so the row-filtered values of rows rc - 1, rc,
        // rc + 1 (reflected at the image border like the pyramid kernel's) are kept and one new row is filtered per
        // new rc; fetch3() only issues the loads of a row's three bytes (four rows ahead, like the float loads).
        const int xl = FRAME ? reflect101(xc - 1, W) : 0, xr = FRAME ? reflect101(xc + 1, W) : 0;
        using RawPx = std::conditional_t<std::is_signed<SRC>::value, int, unsigned>;   // exact: sign- / zero-extended
        struct Raw3 {
            RawPx l, c, r;
        };
        auto fetch3 = [&](int srow) {   // srow: a row of the frame
            const SRC* rp = reinterpret_cast<const SRC*>(sb + (ptrdiff_t)srow * srs);
            return Raw3{rp[xl], rp[xc], rp[xr]};
        };
        auto hval = [&](const Raw3& q) { return nsof_madd<false>((float)q.l + (float)q.r, fr.k1, (float)q.c * fr.k0); };
        int rc_cur = 0;
        float hm = 0.f, h0 = 0.f, hp = 0.f, icur = 0.f;
        auto below = [&](int row) { return reflect101(clampi(row, 0, H - 1) + 1, H); };   // the frame row under clamp(row)
        auto advance = [&](int row, const Raw3& under) {   // I[clamp(row)][xc]; under = fetch3(below(row))
            const int rc = clampi(row, 0, H - 1);
            if (rc != rc_cur) {   // block-uniform; rows come in order: rc == rc_cur + 1
                hm = h0;
                h0 = hp;
                hp = hval(under);
                icur = nsof_madd<false>(hm + hp, fr.k1, h0 * fr.k0);
                rc_cur = rc;
            }
            return icur;
        };
        float win[2 * N + 1];   // win[j] = I[clamp(y - N + j)][xc]
        float pre[4];
        Raw3 praw[4];
        if constexpr (FRAME) {
            rc_cur = clampi(ys - N, 0, H - 1);
            hm = hval(fetch3(reflect101(rc_cur - 1, H)));
            h0 = hval(fetch3(rc_cur));
            hp = hval(fetch3(reflect101(rc_cur + 1, H)));
            icur = nsof_madd<false>(hm + hp, fr.k1, h0 * fr.k0);
            win[0] = icur;
#pragma unroll
            for (int j = 1; j <= 2 * N; j++) win[j] = advance(ys - N + j, fetch3(below(ys - N + j)));
#pragma unroll
            for (int q = 0; q < 4; q++) pre[q] = advance(ys + 1 + N + q, fetch3(below(ys + 1 + N + q)));
        } else {
#pragma unroll
            for (int j = 0; j <= 2 * N; j++) win[j] = ld(ys - N + j);
#pragma unroll
            for (int q = 0; q < 4; q++) pre[q] = ld(ys + 1 + N + q);
        }
        for (int t = 0; t <= nsteps; t++) {
            if (t < nsteps) {
                const int y = ys + 4 * t, buf = t & 1;
                float nxt[4];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if constexpr (FRAME) praw[q] = fetch3(below(y + 5 + N + q));
                    else nxt[q] = ld(y + 5 + N + q);
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    float t0 = win[N] * tp.g[0], t1 = 0.f, t2 = 0.f;
#pragma unroll
                    for (int k = 1; k <= N; k++) {
                        const float a = win[N - k], b = win[N + k];
                        float p = a + b;
                        t0 = t0 + tp.g[k] * p;
                        t2 = t2 + tp.xxg[k] * p;
                        p = b - a;
                        t1 = t1 + tp.xg[k] * p;
                    }
                    sr[buf][0][q][tid] = t0;
                    sr[buf][1][q][tid] = t1;
                    sr[buf][2][q][tid] = t2;
#pragma unroll
                    for (int j = 0; j < 2 * N; j++) win[j] = win[j + 1];
                    win[2 * N] = pre[q];
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if constexpr (FRAME) pre[q] = advance(y + 5 + N + q, praw[q]);
                    else pre[q] = nxt[q];
                }
            }
            __syncthreads();
        }
        return;
    }

    // ---- horizontal pass: wave <-> row, lane <-> 4 pixels, one step behind the vertical pass
    char* Rb = reinterpret_cast<char*>(R + r_off);
    for (int t = 0; t <= nsteps; t++) {
        if (t >= 1) {
            const int y = ys + 4 * (t - 1), buf = (t - 1) & 1;
            const int yo = y + wave;
            const int xo = x0 + 4 * lane;
            if (4 * lane < G::SW && yo < ye && xo < W) {
                const unsigned opix = (unsigned)yo * (unsigned)W + (unsigned)xo;
                auto load_row = [&](int a, float (&v)[4 * G::NV]) {
                    const float4* p4 = reinterpret_cast<const float4*>(&sr[buf][a][wave][4 * lane]);
#pragma unroll
                    for (int i = 0; i < G::NV; i++) {
                        const float4 f = p4[i];
                        v[4 * i] = f.x; v[4 * i + 1] = f.y; v[4 * i + 2] = f.z; v[4 * i + 3] = f.w;
                    }
                };
                // each output goes out (to the transpose planes, or to memory) as soon as it is final, and moment row 2
                // is taken before row 1 so that b1 * ig03 dies early: the live set stays one tap row plus the sums
                auto put = [&](int c, const float (&o)[4]) {   // lane's 4 pixels of channel c: one conflict-free ds_write_b128
                    *reinterpret_cast<float4*>(&st[wave][c][4 * lane]) = make_float4(o[0], o[1], o[2], o[3]);
                };
                double t03[4];  // b1 * ig03, shared by the xx and yy outputs
                {
                    float v[4 * G::NV], o1[4], o3[4];
                    load_row(0, v);
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const int c = G::NP + p;
                        double a1 = (double)(v[c] * tp.g[0]), a2 = 0, a4 = 0;
#pragma unroll
                        for (int k = 1; k <= N; k++) {
                            const float hi = v[c + k], lo = v[c - k];
                            const double tg = (double)(hi + lo);
                            a1 = fma(tg, tp.dg[k], a1);     // product of two float-valued doubles is exact
                            a4 = fma(tg, tp.dxxg[k], a4);
                            a2 += (double)((hi - lo) * tp.xg[k]);
                        }
                        t03[p] = a1 * tp.ig03;
                        o1[p] = (float)(a2 * tp.ig11);
                        o3[p] = (float)(t03[p] + a4 * tp.ig33);
                    }
                    put(1, o1);
                    put(3, o3);
                }
                {
                    float v[4 * G::NV], o2[4];
                    load_row(2, v);
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const int c = G::NP + p;
                        double a5 = (double)(v[c] * tp.g[0]);
#pragma unroll
                        for (int k = 1; k <= N; k++) a5 += (double)((v[c + k] + v[c - k]) * tp.g[k]);
                        o2[p] = (float)(t03[p] + a5 * tp.ig33);
                    }
                    put(2, o2);
                }
                {
                    float v[4 * G::NV], o0[4], o4[4];
                    load_row(1, v);
#pragma unroll
                    for (int p = 0; p < 4; p++) {
                        const int c = G::NP + p;
                        double a3 = (double)(v[c] * tp.g[0]), a6 = 0;
#pragma unroll
                        for (int k = 1; k <= N; k++) {
                            const float hi = v[c + k], lo = v[c - k];
                            a3 += (double)((hi + lo) * tp.g[k]);
                            a6 += (double)((hi - lo) * tp.xg[k]);
                        }
                        o0[p] = (float)(a3 * tp.ig11);
                        o4[p] = (float)(a6 * tp.ig55);
                    }
                    put(0, o0);
                    float* c4 = reinterpret_cast<float*>(Rb) + 4u * plane + opix;
                    if ((W & 3) == 0) {
                        nsof_store_stream4(c4, o4[0], o4[1], o4[2], o4[3]);
                    } else {
#pragma unroll
                        for (int p = 0; p < 4; p++)
                            if (xo + p < W) c4[p] = o4[p];
                    }
                }
            }
            {
                // every lane of the wave takes part (lanes beyond the strip read slots nobody wrote, and do not store)
                float4* q4 = reinterpret_cast<float4*>(Rb) + (unsigned)yo * (unsigned)W + (unsigned)x0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int px = 64 * k + lane;   // pixel within the strip row
                    const float* s = &st[wave][0][px];
                    if (px < G::SW && yo < ye && x0 + px < W) nsof_store_stream4(reinterpret_cast<float*>(q4 + px), s[0], s[256], s[512], s[768]);
                }
            }
        }
        __syncthreads();
    }
}

template <int N, typename SRC = uint8_t>
void launch_polyexp_n(nsof_ctx* ctx, int n_img, const float* img, int W, int H, const nsof_poly_taps& taps, float* R,
                      const PolyFrame* fr = nullptr)
{
    using G = PolyGeom<N>;
    const int strips = (W + G::SW - 1) / G::SW;
    // segment the height so that the grid has >= ~2048 blocks, but keep segments >= 64 rows
    int segs = 1;
    while (segs < 64 && (long long)strips * n_img * segs < 2048 && (H / (segs * 2)) >= 64) segs *= 2;
    // a lone pair: segments down to 16 rows (each re-loads 2N+1 rows of warm-up) until there is a workgroup per CU
    while (segs < 128 && (long long)strips * n_img * segs < 256 && (H / (segs * 2)) >= 16) segs *= 2;
    int seg_rows = ((H + segs - 1) / segs + 3) / 4 * 4;
    segs = (H + seg_rows - 1) / seg_rows;
    dim3 grid(strips, segs, n_img);
    if (fr)
        hipLaunchKernelGGL((k_polyexp_rs<N, false, true, SRC>), grid, dim3(512), 0, ctx->stream, img, R, W, H, seg_rows, taps, nullptr, *fr);
    else if (ctx->opt_polyexp_f32)
        hipLaunchKernelGGL((k_polyexp<N>), grid, dim3(256), 0, ctx->stream, img, R, W, H, seg_rows, taps, nullptr);
    else
        hipLaunchKernelGGL((k_polyexp_rs<N, false>), grid, dim3(512), 0, ctx->stream, img, R, W, H, seg_rows, taps, nullptr);
}

// Work-list twin: W, H are the largest level extents over the table, n_img = 2 * items.
template <int N, typename SRC = uint8_t>
void launch_polyexp_het_n(nsof_ctx* ctx, int n_img, const nsof_het_item* items, const float* img, int W, int H,
                          const nsof_poly_taps& taps, float* R, const PolyFrame* fr = nullptr)
{
    using G = PolyGeom<N>;
    const int strips = (W + G::SW - 1) / G::SW;
    int segs = 1;
    while (segs < 64 && (long long)strips * n_img * segs < 2048 && (H / (segs * 2)) >= 64) segs *= 2;
    int seg_rows = ((H + segs - 1) / segs + 3) / 4 * 4;
    segs = (H + seg_rows - 1) / seg_rows;
    dim3 grid(strips, segs, n_img);
    if (fr) hipLaunchKernelGGL((k_polyexp_rs<N, true, true, SRC>), grid, dim3(512), 0, ctx->stream, img, R, W, H, seg_rows, taps, items, *fr);
    else hipLaunchKernelGGL((k_polyexp_rs<N, true>), grid, dim3(512), 0, ctx->stream, img, R, W, H, seg_rows, taps, items);
}

// f(N) with the radius N of taps as a constant, for the launchers below.
template <class Fn>
int with_poly_n(nsof_ctx* ctx, const nsof_poly_taps& taps, Fn&& f)
{
    if (!nsof_with_int<1, NSOF_MAX_POLY_N>(taps.n, f))
        return nsof_set_error(ctx, NSOF_EUNSUPPORTED, "poly_n=%d outside 1..%d", taps.n, NSOF_MAX_POLY_N);
    NSOF_HIP(ctx, hipGetLastError());
    return NSOF_OK;
}
int not_integer(nsof_ctx* ctx) { return nsof_set_error(ctx, NSOF_EINVAL, "fused level 0 takes integer frames only"); }

}  // namespace

// The expansion of the full-resolution level straight from the integer frames (k_polyexp_rs<.., FRAME, SRC>): images
// [0, nsplit) at src0 + z * img_stride, the rest at src1; k0 / k1 = centre / side tap of the level's 3-tap smoothing.
int nsof_launch_polyexp_frames(nsof_ctx* ctx, int n_img, const void* src0, const void* src1, int nsplit, ptrdiff_t row_stride,
                           ptrdiff_t img_stride, int W, int H, const nsof_poly_taps& taps, float k0, float k1, float* R,
                           int src_type)
{
    nsof_prof_scope ps(ctx, NSOF_K_POLYEXP);
    const PolyFrame fr{static_cast<const uint8_t*>(src0), static_cast<const uint8_t*>(src1), (long long)row_stride,
                    (long long)img_stride, nsplit, k0, k1};
    int rc = NSOF_OK;
    const bool known = nsof_with_src_type(src_type, [&](auto px_tag) {
        using SRC = typename decltype(px_tag)::type;
        if constexpr (std::is_integral<SRC>::value)
            rc = with_poly_n(ctx, taps, [&](auto n) { launch_polyexp_n<decltype(n)::value, SRC>(ctx, n_img, nullptr, W, H, taps, R, &fr); });
        else
            rc = not_integer(ctx);
    });
    return known ? rc : not_integer(ctx);
}

int nsof_launch_polyexp(nsof_ctx* ctx, int n_img, const float* img, int W, int H, const nsof_poly_taps& taps, float* R)
{
    nsof_prof_scope ps(ctx, NSOF_K_POLYEXP);
    return with_poly_n(ctx, taps, [&](auto n) { launch_polyexp_n<decltype(n)::value>(ctx, n_img, img, W, H, taps, R); });
}

// blur3: non-null at the full-resolution level = form the level image from the items' own frames (k0, k1 = centre / side
// tap); I is not read then.
// src_type: the items' pixel type (read only with blur3: 8- or 16-bit).
int nsof_launch_polyexp_het(nsof_ctx* ctx, int n_items, const nsof_het_item* d_items, int max_w, int max_h,
                            const nsof_poly_taps& taps, const float* I, float* R, const float* blur3, int src_type)
{
    nsof_prof_scope ps(ctx, NSOF_K_POLYEXP);
    const int nz = 2 * n_items;
    PolyFrame frv{};
    if (blur3) { frv.k0 = blur3[0]; frv.k1 = blur3[1]; }
    const PolyFrame* fr = blur3 ? &frv : nullptr;
    int rc = NSOF_OK;
    const bool known = nsof_with_src_type(blur3 ? src_type : NSOF_SRC_U8, [&](auto px_tag) {
        using SRC = typename decltype(px_tag)::type;
        if constexpr (std::is_integral<SRC>::value)
            rc = with_poly_n(ctx, taps, [&](auto n) { launch_polyexp_het_n<decltype(n)::value, SRC>(ctx, nz, d_items, I, max_w, max_h, taps, R, fr); });
        else
            rc = not_integer(ctx);
    });
    return known ? rc : not_integer(ctx);
}
