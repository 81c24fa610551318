// csprng.h — the randomness behind keygen and encrypt (host side, outside execute()).
//
// The reference takes its randomness from SEAL's default UniformRandomGeneratorFactory (a BLAKE2
// XOF seeded with 512 bits of OS entropy, reached from /root/reference/eva/seal/seal.cpp:85
// `encryptor.encrypt` and :188-196 `KeyGenerator`).  Here: ChaCha20 (RFC 8439 block function) as
// a counter-mode generator keyed with 256 bits from getrandom(2) — one independent stream per
// keygen and per encrypt call.  A caller-supplied 64-bit seed (generate_keys(params, seed != 0))
// gives a reproducible stream for tests and is NOT secret-grade: 64 bits of key.
#pragma once
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <sys/random.h>

namespace evahost {

// RFC 8439 section 2.3 block function: out = the 16 words of the block for the state `in`
inline void chacha20_block(const uint32_t in[16], uint32_t out[16]) {
  auto rotl = [](uint32_t x, int r) { return (x << r) | (x >> (32 - r)); };
  auto quarter = [&](uint32_t *s, int a, int b, int c, int d) {
    s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 16);
    s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 12);
    s[a] += s[b]; s[d] = rotl(s[d] ^ s[a], 8);
    s[c] += s[d]; s[b] = rotl(s[b] ^ s[c], 7);
  };
  std::memcpy(out, in, 64);
  for (int r = 0; r < 10; r++) {
    quarter(out, 0, 4, 8, 12); quarter(out, 1, 5, 9, 13); quarter(out, 2, 6, 10, 14); quarter(out, 3, 7, 11, 15);
    quarter(out, 0, 5, 10, 15); quarter(out, 1, 6, 11, 12); quarter(out, 2, 7, 8, 13); quarter(out, 3, 4, 9, 14);
  }
  for (int i = 0; i < 16; i++) out[i] += in[i];
}

// Limb `prime` (the chain index) of the uniform polynomial a of a seeded symmetric ciphertext, in NTT
// form as stored: coefficient j = (hi 2^64 + lo) mod q with (lo, hi) = u64 words 2 (j % 4), 2 (j % 4) + 1 of the
// ChaCha20 block with key = seed, block counter j / 4 (state words 12-13), nonce 0x6331000000000000 | prime (words
// 14-15).  No rejection: the bias is below q / 2^128.  The device twin is csrc/seeded.hip.
inline void seeded_limb(const uint8_t seed[32], uint32_t prime, uint64_t q, uint32_t N, uint64_t *out) {
  static const uint32_t sigma[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  uint32_t st[16], w[16];
  std::memcpy(st, sigma, 16);
  std::memcpy(st + 4, seed, 32);
  const uint64_t nonce = 0x6331000000000000ull | prime;
  st[14] = (uint32_t)nonce;
  st[15] = (uint32_t)(nonce >> 32);
  for (uint32_t j0 = 0; j0 < N; j0 += 4) {
    const uint64_t blk = j0 / 4;
    st[12] = (uint32_t)blk;
    st[13] = (uint32_t)(blk >> 32);
    chacha20_block(st, w);
    for (uint32_t r = 0; r < 4 && j0 + r < N; r++) {
      const uint64_t lo = (uint64_t)w[4 * r] | ((uint64_t)w[4 * r + 1] << 32), hi = (uint64_t)w[4 * r + 2] | ((uint64_t)w[4 * r + 3] << 32);
      out[j0 + r] = (uint64_t)((((unsigned __int128)hi << 64) | lo) % q);
    }
  }
}

// Small polynomial p of the value whose 32-byte randomness key is rk: p = 0 the ternary u, p = 1 the
// error e0 (the one error of a symmetric encryption), p = 2 the error e1.  Coefficient j takes the little-endian u64
// word w = j % 8 of the ChaCha20 block with key = rk, block counter j / 8 (state words 12-13), nonce
// 0x736d000000000000 | p (words 14-15).  Ternary: floor(3 w / 2^64) - 1, no rejection, every outcome within 2^-64 of
// 1/3.  Error: HostContext::sample_error's rule on w.  The device twin is csrc/sampled.hip.h.
inline void sampled_small(const uint8_t rk[32], uint32_t p, uint32_t N, int8_t *out) {
  static const uint32_t sigma[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  uint32_t st[16], w[16];
  std::memcpy(st, sigma, 16);
  std::memcpy(st + 4, rk, 32);
  const uint64_t nonce = 0x736d000000000000ull | p;
  st[14] = (uint32_t)nonce;
  st[15] = (uint32_t)(nonce >> 32);
  for (uint32_t j0 = 0; j0 < N; j0 += 8) {
    const uint64_t blk = j0 / 8;
    st[12] = (uint32_t)blk;
    st[13] = (uint32_t)(blk >> 32);
    chacha20_block(st, w);
    for (uint32_t r = 0; r < 8 && j0 + r < N; r++) {
      const uint64_t x = (uint64_t)w[2 * r] | ((uint64_t)w[2 * r + 1] << 32);
      out[j0 + r] = p == 0 ? (int8_t)((int)(uint64_t)(((unsigned __int128)x * 3) >> 64) - 1)
                           : (int8_t)(__builtin_popcountll(x & 0x1FFFFF) - __builtin_popcountll((x >> 21) & 0x1FFFFF));
    }
  }
  volatile uint32_t *v = st; // the key and the last block do not stay on the stack
  for (int i = 0; i < 16; i++) v[i] = 0;
  v = w;
  for (int i = 0; i < 16; i++) v[i] = 0;
}

// The flooding noise of a decryption share from its 32-byte key fk: coefficient j takes the little-endian
// u64 word w = j % 8 of the ChaCha20 block with key = fk, block counter j / 8 (state words 12-13), nonce
// 0x666c000000000000 (words 14-15; a tag of its own beside 0x6331... of the seeded polynomials and 0x736d... of the small
// ones).  E_j = (int64)(w >> (63 - sigma)) - 2^sigma: exactly uniform on [-2^sigma, 2^sigma), no rejection,
// 1 <= sigma <= 62.  A shorter N is a prefix.  The device twin is csrc/sampled.hip.h flood_block.
constexpr uint64_t FLOOD_NONCE = 0x666c000000000000ull;
inline void flood_wide(const uint8_t fk[32], uint32_t sigma, uint32_t N, int64_t *out) {
  if (sigma < 1 || sigma > 62) throw std::invalid_argument("smudge_bits must be 1..62");
  static const uint32_t sg[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  uint32_t st[16], w[16];
  std::memcpy(st, sg, 16);
  std::memcpy(st + 4, fk, 32);
  st[14] = (uint32_t)FLOOD_NONCE;
  st[15] = (uint32_t)(FLOOD_NONCE >> 32);
  for (uint32_t j0 = 0; j0 < N; j0 += 8) {
    const uint64_t blk = j0 / 8;
    st[12] = (uint32_t)blk;
    st[13] = (uint32_t)(blk >> 32);
    chacha20_block(st, w);
    for (uint32_t r = 0; r < 8 && j0 + r < N; r++) {
      const uint64_t x = (uint64_t)w[2 * r] | ((uint64_t)w[2 * r + 1] << 32);
      out[j0 + r] = (int64_t)(x >> (63 - sigma)) - ((int64_t)1 << sigma);
    }
  }
  volatile uint32_t *v = st; // the key and the last block do not stay on the stack
  for (int i = 0; i < 16; i++) v[i] = 0;
  v = w;
  for (int i = 0; i < 16; i++) v[i] = 0;
}

// The common seed of digit J's public rows a_J in the collective relinearization-key generation: the
// first 32 bytes of the ChaCha20 block with key = the digit's PUBLIC relinearization-key seed (equal across the parties of
// one common_seed), block counter 0 and the 8-byte nonce "evarlk\0\0" (state words 14-15, beside "evacrs\0\0" of the
// common stream and the tags 0x6331 / 0x736d / 0x666c of the expansions).  It must differ from its input: a party's own
// relinearization key publishes c0 = -(a s_p + e) + w s_p^2 under the input seed's a, and a round-1 share a s_p + e1 under
// the SAME a would cancel a s_p and leave w s_p^2 plus small noise in the open.  The one derivation of the host and of
// the callers of evah_keygen_relin_round1.
inline void relin_round_seed(const uint8_t relin_seed[32], uint8_t out[32]) {
  static const uint32_t sigma[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
  uint32_t st[16], w[16];
  std::memcpy(st, sigma, 16);
  std::memcpy(st + 4, relin_seed, 32);
  st[12] = st[13] = 0;
  std::memcpy(st + 14, "evarlk\0\0", 8);
  chacha20_block(st, w);
  std::memcpy(out, w, 32);
}

class SecureRng {
public:
  using result_type = uint64_t;
  static constexpr result_type min() { return 0; }
  static constexpr result_type max() { return ~(result_type)0; }

  SecureRng() { // 256-bit key + 64-bit nonce from the operating system
    unsigned char seed[40];
    size_t got = 0;
    while (got < sizeof seed) {
      ssize_t r = getrandom(seed + got, sizeof seed - got, 0);
      if (r < 0) throw std::runtime_error("getrandom failed: no entropy source for key generation / encryption");
      got += (size_t)r;
    }
    init(seed, seed + 32);
    wipe(seed, sizeof seed);
  }
  explicit SecureRng(uint64_t test_seed, uint64_t stream = 0) { // reproducible test hook
    unsigned char key[32] = {0}, nonce[8];
    std::memcpy(key, &test_seed, 8);
    std::memcpy(key + 8, "eva_amd test seed: not secret", 24);
    std::memcpy(nonce, &stream, 8);
    init(key, nonce);
  }
  // the common public stream of a collective key generation: every party that keys it with the same 32
  // bytes draws the same seeds; nothing secret comes from it
  struct CommonSeed { const uint8_t *key32; };
  explicit SecureRng(CommonSeed cs) { init(cs.key32, reinterpret_cast<const unsigned char *>("evacrs\0\0")); }
  ~SecureRng() { wipe(state_, sizeof state_); wipe(block_, sizeof block_); }
  SecureRng(const SecureRng &) = delete;
  SecureRng &operator=(const SecureRng &) = delete;

  result_type operator()() {
    if (pos_ == 8) refill();
    return block_[pos_++];
  }

private:
  uint32_t state_[16];
  uint64_t block_[8];
  int pos_ = 8;

  static void wipe(void *p, size_t n) {
    volatile unsigned char *v = static_cast<volatile unsigned char *>(p);
    while (n--) *v++ = 0;
  }
  void init(const unsigned char *key, const unsigned char *nonce8) {
    static const uint32_t sigma[4] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u};
    std::memcpy(state_, sigma, 16);
    std::memcpy(state_ + 4, key, 32);
    state_[12] = state_[13] = 0; // 64-bit block counter
    std::memcpy(state_ + 14, nonce8, 8);
  }
  void refill() {
    uint32_t w[16];
    chacha20_block(state_, w);
    std::memcpy(block_, w, sizeof block_);
    wipe(w, sizeof w);
    if (++state_[12] == 0) ++state_[13];
    pos_ = 0;
  }
};

} // namespace evahost
