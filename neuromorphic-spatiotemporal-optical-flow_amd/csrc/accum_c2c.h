// Cycle-to-cycle write noise: the counter generator and the variate both accumulators draw from (include/nsof.h states the
// definition).  Shared by the event-driven trial run (accum_trials.hip: one draw per update of a slice) and the frame-driven
// run (accum_frames.hip: one draw per frame pair).  Integer arithmetic and one rounded multiply: host and device agree.
#pragma once

#include <hip/hip_runtime.h>

// Philox4x32-10 (Salmon et al., SC'11): c <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)) ten times,
// the key bumped by the Weyl constants after each of the first nine rounds.  Integer arithmetic only: host and device agree.
__host__ __device__ inline void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
    constexpr unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)M0 * c[0], p1 = (unsigned long long)M1 * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (unsigned)p1; c[2] = n2; c[3] = (unsigned)p0;
        k0 += W0; k1 += W1;   // (the bump after the tenth round is never read)
    }
}
// The variate of one update: counter (pixel, slice low, slice high, trial + 65536 * array), key = the seed's two words; S =
// the sum of the 16 output bytes (0..4080, Irwin-Hall(16) on bytes: mean 2040, variance 87380), xi = float(S - 2040) * c
// with c = float32(1 / sqrt(87380)): one exact conversion and one rounded multiply.  The bytes are summed two per 16-bit
// lane (8 * 255 fits), then the lanes: plain integer code, the same on both sides.
__host__ __device__ inline float c2c_xi(unsigned k0, unsigned k1, unsigned pixel, unsigned long long slice, unsigned trial_word)
{
    unsigned c[4] = {pixel, (unsigned)slice, (unsigned)(slice >> 32), trial_word};
    philox4x32_10(c, k0, k1);
    unsigned lanes = 0;
    for (int i = 0; i < 4; i++) lanes += (c[i] & 0x00ff00ffu) + ((c[i] >> 8) & 0x00ff00ffu);
    const int sum = (int)((lanes & 0xffffu) + (lanes >> 16));
    return (float)(sum - 2040) * 0x1.bb688cp-9f;
}
__host__ __device__ inline unsigned c2c_trial_word(int array, int trial) { return (unsigned)trial + 65536u * (unsigned)array; }
