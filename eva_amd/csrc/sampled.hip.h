// sampled.hip.h — the small polynomials of an encryption drawn on the device from a 32-byte randomness key per value
// (DESIGN.md 1.7), used by client.hip: polynomial p (0 = the ternary u, 1 = the error e0 — the one error of a
// symmetric encryption —, 2 = the error e1), coefficient j from the little-endian u64 word w = j % 8 of the ChaCha20
// block of key = the randomness key, block counter = j / 8 (state words 12-13), nonce = 0x736d000000000000 | p (words
// 14-15).  Ternary: floor(3 w / 2^64) - 1 (no rejection, every outcome within 2^-64 of 1/3); error:
// popcount(w & 0x1FFFFF) - popcount((w >> 21) & 0x1FFFFF), the host sampler's rule.  A polynomial depends only on
// (key, p).  Host twin: eva_amd/host/csprng.h sampled_small.
#pragma once
#include "seeded.hip.h"

namespace evah {

constexpr uint32_t SAMPLE_NONCE_HI = 0x736d0000u;

// the 8 small coefficients of block `blk` of polynomial p, as the bytes of one u64 (coefficient 8 blk + r in byte r)
__device__ __forceinline__ u64 sampled_block(const uint32_t *key, uint32_t p, uint64_t blk) {
  uint32_t x[16];
  chacha_block(key, blk, p, SAMPLE_NONCE_HI, x);
  u64 packed = 0;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const u64 w = chacha_w64(x, r);
    const int v = p == 0 ? (int)__umul64hi(w, 3) - 1 : __popcll(w & 0x1FFFFF) - __popcll((w >> 21) & 0x1FFFFF);
    packed |= (u64)(uint8_t)(int8_t)v << (8 * r);
  }
  return packed;
}

// The flooding noise of a decryption share: coefficient j of the noise of key fk from the little-endian
// u64 word w = j % 8 of the ChaCha20 block of key = fk, block counter = j / 8, nonce = 0x666c000000000000 (a tag of its
// own: no block is shared with a seeded polynomial or a small one).  E = (w >> (63 - sigma)) - 2^sigma, exactly uniform
// on [-2^sigma, 2^sigma) for 1 <= sigma <= 62, no rejection.  Host twin: eva_amd/host/csprng.h flood_wide.
constexpr uint32_t FLOOD_NONCE_HI = 0x666c0000u;

__device__ __forceinline__ void flood_block(const uint32_t *key, uint32_t sigma, uint64_t blk, int64_t e[8]) {
  uint32_t x[16];
  chacha_block(key, blk, 0, FLOOD_NONCE_HI, x);
#pragma unroll
  for (int r = 0; r < 8; r++) e[r] = (int64_t)(chacha_w64(x, r) >> (63 - sigma)) - ((int64_t)1 << sigma);
}

} // namespace evah
