// The counter-based random streams of libhsp (gfx950), stated once: Philox4x32-10 and the normal draw built on it.
// hsp_plm.hip draws the sampled PLM decision from the words themselves (hsp.h "sampled PLM decoding", counters
// (i >> 2, j, 0, 0)); hsp_pointwise.hip draws the prior noise through hsp_normal4 (hsp.h "seeded prior noise", counters
// (t >> 2, c, 0, 1)).  The last counter word names the stream, so one seed serves both without a shared word.
#pragma once
#include "hsp_device.h"

// Philox4x32-10 (Random123): counter c[0..3] -> four words in place, under the key (k0, k1)
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const unsigned lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

// THE normal draw of hsp.h "seeded prior noise": n[k] = the standard normal of frame 4 g + k of channel c under `seed`.
// One Philox call; the word pairs (w0, w1) and (w2, w3) each give one Box-Muller pair.  u1 = ((wa >> 9) + 0.5) 2^-23 in
// (0, 1) and 2 u2 = (wb >> 8) 2^-23 in [0, 2) are exact in fp32; cos / sin of 2 pi u2 are taken as cospi / sinpi of
// 2 u2, so no rounded 2 pi enters.  |n| <= sqrt(48 ln 2) = 5.768.  Every kernel that needs the noise calls this one
// function, so the same (seed, c, t) gives the same bits wherever it is drawn.
__device__ __forceinline__ void hsp_normal4(int64_t seed, unsigned c, unsigned g, float n[4]) {
  unsigned w[4] = {g, c, 0u, 1u};
  philox4x32_10(w, (unsigned)(uint64_t)seed, (unsigned)((uint64_t)seed >> 32));
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float u1 = ((float)(w[2 * p] >> 9) + 0.5f) * 0x1p-23f;
    const float u2x2 = (float)(w[2 * p + 1] >> 8) * 0x1p-23f;
    const float r = sqrtf(-2.0f * logf(u1));
    float sn, cs;
    sincospif(u2x2, &sn, &cs);
    n[2 * p] = r * cs;
    n[2 * p + 1] = r * sn;
  }
}
