// client.hip.h — what client.hip (one ciphertext per call) and client_batch.hip (a batch per call) share: the Garner
// tables of a level and the exact recomposition of a decrypted coefficient to one double (SEAL 3.6
// CKKSEncoder::decode_internal).  One definition, so that both paths give the same doubles by construction.
#pragma once
#include "launch.hip.h"

namespace evah {

// Garner tables of a level: inv_prefix[i] = (q_0..q_{i-1})^-1 mod q_i, pre_mod[i][t] = q_0..q_{t-1} mod q_i,
// prefix[i][w] = word w of q_0..q_{i-1} (base 2^64, l words), qwords[w] / half[w] = word w of Q / of floor(Q/2)
struct CrtTab {
  const u64 *inv_prefix, *pre_mod, *prefix, *qwords, *half;
};
// the tables in one array of 2 l^2 + 3 l words: [inv_prefix l][pre_mod l*l][prefix l*l][Q l][floor(Q/2) l]
inline size_t crt_tab_words(uint32_t l) { return (size_t)2 * l * l + 3 * l; }
inline CrtTab crt_tab_at(const u64 *d, uint32_t l) {
  return CrtTab{d, d + l, d + l + (size_t)l * l, d + l + (size_t)2 * l * l, d + 2 * l + (size_t)2 * l * l};
}
inline std::vector<u64> crt_tab_build(const evah_ctx *c, uint32_t l) {
  std::vector<u64> tab(crt_tab_words(l), 0);
  u64 *inv_prefix = tab.data(), *pre_mod = inv_prefix + l, *prefix = pre_mod + (size_t)l * l,
      *qwords = prefix + (size_t)l * l, *half = qwords + l;
  std::vector<u64> w{1}; // q_0..q_{i-1}, little-endian words
  for (uint32_t i = 0; i < l; i++) {
    const u64 qi = c->primes[i];
    u64 acc = 1 % qi;
    for (uint32_t j = 0; j < i; j++) {
      pre_mod[i * l + j] = acc;
      acc = mulmod(acc, c->primes[j] % qi, qi);
    }
    inv_prefix[i] = invmod(acc, qi);
    for (size_t t = 0; t < w.size() && t < l; t++) prefix[(size_t)i * l + t] = w[t];
    u64 carry = 0;
    for (auto &x : w) { u128 t = (u128)x * qi + carry; x = (u64)t; carry = (u64)(t >> 64); }
    if (carry) w.push_back(carry);
  }
  for (size_t t = 0; t < w.size() && t < l; t++) qwords[t] = w[t];
  for (size_t t = 0; t < w.size() && t < l; t++) half[t] = (w[t] >> 1) | (t + 1 < w.size() ? w[t + 1] << 63 : 0);
  return tab;
}

__device__ __forceinline__ void garner(const DevCtx &cx, const CrtTab &t, uint32_t l, const u64 *r, u64 *v) {
  for (uint32_t i = 0; i < l; i++) {
    const DevPrime pm = cx.primes[i];
    u128_t acc = {0, 0};
    for (uint32_t j = 0; j < i; j++) acc128(acc, v[j] >= pm.q ? barrett64(v[j], pm.q, pm.brt) : v[j], t.pre_mod[i * l + j]);
    const u64 a = barrett128(acc, pm);
    v[i] = i ? mulmod(submod(r[i], a, pm.q), t.inv_prefix[i], pm) : r[0];
  }
}
// SEAL 3.6 CKKSEncoder::decode_internal between the inverse NTTs and the FFT: the composed coefficient
// x in [0, Q) as l base-2^64 words (here from the mixed-radix digits: x = sum_i v_i q_0..q_{i-1}, exact),
// then ONE double from the words, least significant first, with inv_scale folded into the running power
// of 2^64; x >= (Q + 1) / 2 is negative and accumulates the signed per-word differences against Q's
// words.  Same operations in the same order as the oracle's evo_decode and the host decoder: same doubles.
// coeff = limb 0 of the message [l][N], n = the coefficient.
__device__ __forceinline__ double crt_to_double(const DevCtx &cx, const CrtTab &t, uint32_t l, const u64 *coeff, size_t n, double inv_scale) {
#pragma clang fp contract(off)
  u64 r[62], v[62], x[63];
  for (uint32_t i = 0; i < l; i++) r[i] = coeff[(size_t)i * cx.N + n];
  garner(cx, t, l, r, v);
  for (uint32_t w = 0; w <= l; w++) x[w] = 0;
  for (uint32_t i = 0; i < l; i++) { // x += v_i * prefix_i (prefix_i has at most i words; the sum stays below Q)
    u64 carry = 0;
    const u64 *pf = t.prefix + (size_t)i * l;
    for (uint32_t w = 0; w < l; w++) {
      u128_t p = mul128(pf[w], v[i]);
      const u64 lo = p.lo + carry;
      u64 hi = p.hi + (lo < carry);
      const u64 sum = x[w] + lo;
      hi += (sum < lo);
      x[w] = sum;
      carry = hi;
    }
  }
  bool negative = false; // x > floor(Q/2), compared from the most significant word
  for (int w = (int)l - 1; w >= 0; w--)
    if (x[w] != t.half[w]) { negative = x[w] > t.half[w]; break; }
  const double two_pow_64 = 18446744073709551616.0;
  double acc = 0.0, scaled = inv_scale;
  for (uint32_t w = 0; w < l; w++, scaled *= two_pow_64) {
    const u64 xw = x[w], qw = t.qwords[w];
    if (!negative) {
      acc += xw ? (double)xw * scaled : 0.0;
    } else if (xw > qw) {
      const u64 diff = xw - qw;
      acc += diff ? (double)diff * scaled : 0.0;
    } else {
      const u64 diff = qw - xw;
      acc -= diff ? (double)diff * scaled : 0.0;
    }
  }
  return acc;
}

// forward roots zeta^br(j) of the decoder's special FFT (hostmath.h), once per context family
inline void dec_tables(evah_ctx *c) {
  if (c->sh->dec_roots) return;
  const uint32_t N = c->N;
  const CkksRoots cr = ckks_roots(N);
  std::vector<double> roots(2 * (size_t)N);
  for (uint32_t j = 0; j < N; j++) { roots[2 * j] = cr.fwd[j].real(); roots[2 * j + 1] = cr.fwd[j].imag(); }
  HIPCHK(hipMalloc(&c->sh->dec_roots, sizeof(double2) * N));
  h2d_now(c, c->sh->dec_roots, roots.data(), sizeof(double2) * N);
}

} // namespace evah
