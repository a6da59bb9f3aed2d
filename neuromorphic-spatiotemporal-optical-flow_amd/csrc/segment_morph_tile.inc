// Body shared by k_morph_bits and k_morph_jobs (included inside both, so that k_morph_bits compiles exactly as it did
// before the job-list kernel existed; an inlined device function changes its code).  In scope: in_bits, wp, w, h,
// el_arg, n_pass, ops, top, rows, out_bits, out_u8, ostride (k_morph_bits' parameters), FIXED10, and TILE_BX / TILE_BY
// (the output tile).  The whole workgroup runs it.
constexpr MorphElem fixed = ellipse10();
const MorphElem& el = FIXED10 ? fixed : el_arg;
extern __shared__ uint32_t lds[];
uint32_t* cur = lds;                       // [rows][TW]
uint32_t* H = lds + (size_t)rows * TW;     // [n_patterns][rows][TW]
const int tid = threadIdx.x;
const int gk0 = TILE_BX * TILE_WORDS - HALO_WORDS;
const int gy0 = TILE_BY * TILE_H - top;
const int n = rows * TW;
const int k = tid & (TW - 1);              // 1024 % TW == 0: a thread keeps its word column
const int gk = gk0 + k;

for (int i = tid; i < n; i += MORPH_THREADS) {
    const int gy = gy0 + (i >> 4);
    cur[i] = (gy >= 0 && gy < h && gk >= 0 && gk < wp) ? in_bits[(size_t)gy * wp + gk] : 0u;
}
__syncthreads();

for (int p = 0; p < n_pass; p++) {
    const bool dil = (ops >> p) & 1u;
    // H step: per distinct row pattern, OR of the funnel-shifted words (one v_alignbit per element column)
    for (int i = tid; i < n; i += MORPH_THREADS) {
        const int gy = gy0 + (i >> 4);
        uint32_t lo = k > 0 ? cur[i - 1] : 0u, mid = cur[i], hi = k + 1 < TW ? cur[i + 1] : 0u;
        if (!dil) {   // complement inside the image; outside stays 0 (= "does not take part" in a minimum)
            lo = k > 0 ? ~lo & inside_bits(gy, gk - 1, w, h) : 0u;
            mid = ~mid & inside_bits(gy, gk, w, h);
            hi = k + 1 < TW ? ~hi & inside_bits(gy, gk + 1, w, h) : 0u;
        }
        h_patterns<0>(el, H, n, i, lo, mid, hi);
    }
    __syncthreads();
    // V step: OR over the element rows of the matching H array
    for (int i = tid; i < n; i += MORPH_THREADS) {
        const int r = i >> 4;
        const uint32_t acc = v_rows<0>(el, H, n, r, k, rows);
        cur[i] = (dil ? acc : ~acc) & inside_bits(gy0 + r, gk, w, h);
    }
    __syncthreads();
}

// write the tile's own rows/words
if (out_u8) {
    for (int i = tid; i < TILE_H * TILE_WORDS * 8; i += MORPH_THREADS) {   // 4 pixels per item
        const int r = i / (TILE_WORDS * 8), q = i - r * (TILE_WORDS * 8);
        const int gy = TILE_BY * TILE_H + r, gx = TILE_BX * TILE_WORDS * 32 + q * 4;
        if (gy >= h || gx >= w) continue;
        const uint32_t word = cur[(r + top) * TW + HALO_WORDS + (q >> 3)];
        const uint32_t nib = (word >> ((q & 7) * 4)) & 0xfu;
        uint8_t* o = out_u8 + (ptrdiff_t)gy * ostride + gx;
        if (gx + 4 <= w && (((uintptr_t)o) & 3) == 0) {
            *(uint32_t*)o = ((nib & 1u) ? 0xffu : 0u) | ((nib & 2u) ? 0xff00u : 0u) | ((nib & 4u) ? 0xff0000u : 0u) |
                            ((nib & 8u) ? 0xff000000u : 0u);
        } else {
            for (int b = 0; b < 4 && gx + b < w; b++) o[b] = (nib >> b) & 1u ? 255 : 0;
        }
    }
} else {
    for (int i = tid; i < TILE_H * TILE_WORDS; i += MORPH_THREADS) {
        const int r = i / TILE_WORDS, kk = i - r * TILE_WORDS;
        const int gy = TILE_BY * TILE_H + r, gk = TILE_BX * TILE_WORDS + kk;
        if (gy < h && gk < wp) out_bits[(size_t)gy * wp + gk] = cur[(r + top) * TW + HALO_WORDS + kk];
    }
}
