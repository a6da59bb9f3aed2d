// Body shared by k_mag_pack and k_mag_pack_jobs (included inside both, so that k_mag_pack compiles exactly as it did
// before the job-list kernel existed; an inlined device function changes its code).  In scope: flow, fstride (floats),
// w, h, thresh, bits, wp, k64 (the row's 64-pixel group), lane, and PACK_BY (the 8-row group).
// One wave packs pixels k64 * 64 .. k64 * 64 + 63 of rows 8 PACK_BY .. 8 PACK_BY + 7: `mag > thresh` -> one ballot per row.
const int x = k64 * 64 + lane;
const int y0 = PACK_BY * 8;
float2 v[8];
#pragma unroll
for (int r = 0; r < 8; r++) {
    const int y = y0 + r;
    v[r] = (x < w && y < h) ? *(const float2*)(flow + (ptrdiff_t)y * fstride + 2 * x) : make_float2(0.f, 0.f);
}
#pragma unroll
for (int r = 0; r < 8; r++) {
    const int y = y0 + r;
    const double a = v[r].x, b = v[r].y;
    const bool set = x < w && y < h && sqrt(a * a + b * b) > thresh;   // cartToPolar on float64, then `mag > th`
    const unsigned long long m = __ballot(set);
    if (lane == 0 && y < h) *(unsigned long long*)(bits + (size_t)y * wp + 2 * k64) = m;
}
