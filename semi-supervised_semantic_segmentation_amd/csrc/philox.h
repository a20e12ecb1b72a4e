// Philox-4x32-10, the counter-based generator behind every device-side random draw (CowMix noise and p / sigma,
// the affine views, the mask family, dropout, the augmentations).  This is the only copy: tests/philox_ref.py restates
// it on the host and tabulates, per consumer, the counter block, the stream word and which output word feeds what.
#pragma once
#include "common.h"

// counter block of draw `ctr`: the 64-bit counter in words 0 and 1, the consumer's stream id (or coordinates) in 2 and 3
__device__ __forceinline__ void philox_block(unsigned (&c)[4], uint64_t ctr, unsigned w2, unsigned w3 = 0u) {
  c[0] = (unsigned)ctr;
  c[1] = (unsigned)(ctr >> 32);
  c[2] = w2;
  c[3] = w3;
}

// ten rounds in place, key = seed, bumped by the Weyl constants after each round
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], uint64_t seed) {
  unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    const unsigned hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const unsigned hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    const unsigned n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the top 24 bits of a word as a uniform: in [0, 1), in (0, 1], and at the cell centres (Box-Muller's log argument)
__device__ __forceinline__ float philox_u01(unsigned w) { return (float)(w >> 8) * (1.0f / 16777216.0f); }
__device__ __forceinline__ float philox_u01_upper(unsigned w) { return ((float)(w >> 8) + 1.0f) * (1.0f / 16777216.0f); }
__device__ __forceinline__ float philox_u01_mid(unsigned w) { return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// the counter offset from device memory (graph-replayable draws: every replay reads the advanced counter) or from the
// argument
__device__ __forceinline__ uint64_t rng_offset(const unsigned long long* dev, uint64_t host, uint64_t add) {
  return (dev ? (uint64_t)*dev : host) + add;
}
