// seeded.hip.h — the expansion of a seeded polynomial, shared by seeded.hip (uploads of c0 + seed)
// and client.hip (k_encrypt_symmetric): limb i (chain prime index), coefficient j = (hi 2^64 + lo) mod q_i with
// (lo, hi) = the words 2 (j % 4) and 2 (j % 4) + 1 (as little-endian u64) of the ChaCha20 block of key = seed, block
// counter = j / 4 (state words 12-13), nonce = 0x6331000000000000 | i (words 14-15).  The result is limb i of c1 in NTT
// form as stored; a limb depends only on (seed, i).  Host twin: eva_amd/host/csprng.h seeded_limb.
#pragma once
#include "launch.hip.h"

namespace evah {

// up to 8 seeds as launch arguments (256 bytes): no host buffer has to outlive the call, and a launch needs no copy
struct Seeds8 {
  uint32_t w[8][8];
};
constexpr uint32_t SEEDS_PER_LAUNCH = 8;
constexpr uint32_t SEED_NONCE_HI = 0x63310000u;

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
#define CHACHA_QR(a, b, c, d)                      \
  a += b; d = rotl32(d ^ a, 16);                   \
  c += d; b = rotl32(b ^ c, 12);                   \
  a += b; d = rotl32(d ^ a, 8);                    \
  c += d; b = rotl32(b ^ c, 7);

// the 16 output words of the ChaCha20 block with key `key`, block counter blk (state words 12-13) and nonce (n0, n1)
// (words 14-15): the one block function of the device, shared with sampled.hip.h
__device__ __forceinline__ void chacha_block(const uint32_t *key, uint64_t blk, uint32_t n0, uint32_t n1, uint32_t x[16]) {
  const uint32_t s0 = 0x61707865u, s1 = 0x3320646eu, s2 = 0x79622d32u, s3 = 0x6b206574u;
  const uint32_t k0 = key[0], k1 = key[1], k2 = key[2], k3 = key[3], k4 = key[4], k5 = key[5], k6 = key[6], k7 = key[7];
  const uint32_t c0 = (uint32_t)blk, c1 = (uint32_t)(blk >> 32);
  uint32_t x0 = s0, x1 = s1, x2 = s2, x3 = s3, x4 = k0, x5 = k1, x6 = k2, x7 = k3;
  uint32_t x8 = k4, x9 = k5, x10 = k6, x11 = k7, x12 = c0, x13 = c1, x14 = n0, x15 = n1;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    CHACHA_QR(x0, x4, x8, x12) CHACHA_QR(x1, x5, x9, x13) CHACHA_QR(x2, x6, x10, x14) CHACHA_QR(x3, x7, x11, x15)
    CHACHA_QR(x0, x5, x10, x15) CHACHA_QR(x1, x6, x11, x12) CHACHA_QR(x2, x7, x8, x13) CHACHA_QR(x3, x4, x9, x14)
  }
  x[0] = x0 + s0; x[1] = x1 + s1; x[2] = x2 + s2; x[3] = x3 + s3; x[4] = x4 + k0; x[5] = x5 + k1; x[6] = x6 + k2; x[7] = x7 + k3;
  x[8] = x8 + k4; x[9] = x9 + k5; x[10] = x10 + k6; x[11] = x11 + k7; x[12] = x12 + c0; x[13] = x13 + c1; x[14] = x14 + n0; x[15] = x15 + n1;
}
#undef CHACHA_QR
__device__ __forceinline__ u64 chacha_w64(const uint32_t x[16], int w) { return (u64)x[2 * w] | ((u64)x[2 * w + 1] << 32); }

// the four coefficients of block `blk` of limb `prime` (the chain index) as canonical residues
__device__ __forceinline__ void seeded_block(const uint32_t *key, uint32_t prime, uint64_t blk, const DevPrime &pm, u64 out[4]) {
  uint32_t x[16];
  chacha_block(key, blk, prime, SEED_NONCE_HI, x);
#pragma unroll
  for (int r = 0; r < 4; r++) out[r] = barrett128(u128_t{chacha_w64(x, 2 * r), chacha_w64(x, 2 * r + 1)}, pm);
}

// the key words of seed z of a launch: from the launch arguments for up to SEEDS_PER_LAUNCH seeds, else from seed_buf
// ([seeds][8] words, uploaded on the same queue) — uniform over the launch
__device__ __forceinline__ void seed_words(const Seeds8 &seeds, const uint32_t *seed_buf, uint32_t z, uint32_t key[8]) {
  if (seed_buf) {
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = seed_buf[8 * z + w];
  } else {
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = seeds.w[z][w];
  }
}

// a thread's four coefficients (one ChaCha block) as two 16-byte accesses; st4_split stores their split30 forms
__device__ __forceinline__ void ld4(const u64 *p, u64 v[4]) {
  const ulonglong2 lo = ld2(p), hi = ld2(p + 2);
  v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
}
__device__ __forceinline__ void st4(u64 *p, const u64 v[4]) {
  st2(p, make_ulonglong2(v[0], v[1]));
  st2(p + 2, make_ulonglong2(v[2], v[3]));
}
__device__ __forceinline__ void st4_split(u64 *p, const u64 v[4]) {
  st2(p, make_ulonglong2(split30(v[0]), split30(v[1])));
  st2(p + 2, make_ulonglong2(split30(v[2]), split30(v[3])));
}

inline Seeds8 seeds_of(const uint8_t *const *seeds, uint32_t first, uint32_t n) {
  Seeds8 s;
  std::memset(&s, 0, sizeof s);
  for (uint32_t z = 0; z < n; z++) {
    if (!seeds[first + z]) throw std::invalid_argument("seed pointer is null");
    std::memcpy(s.w[z], seeds[first + z], 32); // little-endian key words, as the host generator reads its key
  }
  return s;
}
// The seeds of one launch as its kernel takes them (seed_words): n seeds [n][32] (host) as launch arguments, or above
// SEEDS_PER_LAUNCH as a device buffer copied on the queue.  Declare it in the scope that drains the queue: the buffer
// returns to the pool when it ends.
struct SeedArgs {
  Seeds8 s8;
  std::unique_ptr<Scratch> dev;
  const uint32_t *buf = nullptr;
  SeedArgs(evah_ctx *c, const uint8_t *seeds, uint32_t n) {
    std::memset(&s8, 0, sizeof s8);
    if (n <= SEEDS_PER_LAUNCH) {
      std::memcpy(s8.w, seeds, (size_t)32 * n); // little-endian key words, as the host generator reads its key
    } else {
      dev = std::make_unique<Scratch>(c, (size_t)4 * n);
      HIPCHK(hipMemcpyAsync(dev->d, seeds, (size_t)32 * n, hipMemcpyHostToDevice, c->stream));
      buf = reinterpret_cast<const uint32_t *>(dev->d);
    }
  }
};
// client.hip: small polynomials (int8 on the device) to their NTT forms under the first `limbs` chain primes
void small_to_ntt(evah_ctx *c, const u64 *small8, uint32_t n_polys, uint32_t limbs, u64 *out);
// client.hip: the randomness keys rkeys [batch][32] (host) copied into `keys` on the queue, then the NTT forms
// [batch][n_polys][limbs][N] of the small polynomials p0 .. p0 + n_polys - 1 each key expands to
void sample_to_ntt(evah_ctx *c, uint32_t batch, const uint8_t *rkeys, u64 *keys, uint32_t n_polys, uint32_t p0, uint32_t limbs, u64 *out);
// queue-ordered zeroing of a pool temporary that held something secret, also when the call fails
struct Wipe { // shared by client.hip and seeded.hip
  evah_ctx *c;
  void *d;
  size_t bytes;
  bool done = false; // set at construction: nothing to wipe
  void now() { // the success path: a wipe that fails is an error
    if (done) return;
    done = true;
    HIPCHK(hipMemsetAsync(d, 0, bytes, c->stream));
  }
  ~Wipe() {
    if (!done) (void)hipMemsetAsync(d, 0, bytes, c->stream);
  }
};
inline dim3 seeded_grid(const evah_ctx *c, uint32_t limbs, uint32_t z) { return dim3((c->N / 4 + 255) / 256, limbs, z); }

} // namespace evah
