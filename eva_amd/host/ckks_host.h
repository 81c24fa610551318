// ckks_host.h — host-side CKKS (FP64 encoder, key generation, encryption, decryption) for the
// MI355X backend.  These are the once-per-program / once-per-input steps that the reference runs
// through SEAL on the CPU (/root/reference/eva/seal/seal.cpp:24-102 encrypt, :124-146 decrypt,
// :174-203 generateKeys); they stay on the host here too.  execute() never comes through this
// file for ciphertext arithmetic — that is libeva_hip.so.
//
// Algebra follows SURVEY.md Appendix A.9/A.10 (restating SEAL 3.6 CKKSEncoder / KeyGenerator /
// Encryptor / Decryptor).  Randomness is not SEAL's stream; only the algebraic relations matter.
#pragma once
#include <array>
#include <cmath>
#include <complex>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include "csprng.h"
#include "hostmath.h"
#include "../../include/eva_hip.h"

namespace evahost {

using evah::u128;
using evah::u64;

struct HostPrime {
  u64 q = 0, r0 = 0, r1 = 0; // floor(2^128/q)
  u64 ninv = 0, ninv_s = 0;
  std::vector<u64> rp, rps, irp, irps; // heap-ordered root powers + Shoup quotients
};

class HostContext {
public:
  uint32_t N, logN, k;
  std::vector<u64> primes;
  std::vector<HostPrime> pm;
  std::vector<int> total_bits; // total_bits[l] = bit length of q_0...q_{l-1}

  HostContext(uint32_t N_, const std::vector<u64> &primes_) : N(N_), logN(evah::ilog2(N_)), k((uint32_t)primes_.size()), primes(primes_) {
    if (N < 2 || (N & (N - 1))) throw std::invalid_argument("poly_modulus_degree must be a power of two");
    pm.resize(k);
    for (uint32_t i = 0; i < k; i++) {
      HostPrime &m = pm[i];
      m.q = primes[i];
      u128 ratio = (~(u128)0) / m.q;
      m.r0 = (u64)ratio;
      m.r1 = (u64)(ratio >> 64);
      u64 psi = evah::minimal_primitive_root(N, m.q), psi_inv = evah::invmod(psi, m.q);
      m.rp = evah::root_power_table(N, m.q, psi);
      m.irp = evah::root_power_table(N, m.q, psi_inv);
      m.rps.resize(N);
      m.irps.resize(N);
      for (uint32_t j = 0; j < N; j++) {
        m.rps[j] = evah::shoup(m.rp[j], m.q);
        m.irps[j] = evah::shoup(m.irp[j], m.q);
      }
      m.ninv = evah::invmod(N % m.q, m.q);
      m.ninv_s = evah::shoup(m.ninv, m.q);
    }
    std::vector<u64> w{1};
    total_bits.push_back(0);
    for (uint32_t i = 0; i < k; i++) {
      u64 carry = 0;
      for (auto &x : w) {
        u128 t = (u128)x * primes[i] + carry;
        x = (u64)t;
        carry = (u64)(t >> 64);
      }
      if (carry) w.push_back(carry);
      int bits = (int)(w.size() - 1) * 64;
      for (u64 top = w.back(); top; top >>= 1) bits++;
      total_bits.push_back(bits);
    }
    pow2_.resize(k);
    for (uint32_t i = 0; i < k; i++) { // 2^e mod q_i for the encoder's multi-precision residues
      pow2_[i].resize(1100);
      u64 p = 1 % primes[i];
      for (auto &v : pow2_[i]) { v = p; p = evah::addmod(p, p, primes[i]); }
    }
    init_encoder();
  }

  // ---- modular helpers
  static inline u64 mul_shoup_lazy(u64 x, u64 w, u64 ws, u64 q) { return x * w - (u64)(((u128)x * ws) >> 64) * q; }
  inline u64 mulm(u64 a, u64 b, uint32_t i) const {
    const HostPrime &m = pm[i];
    u128 x = (u128)a * b;
    u64 x0 = (u64)x, x1 = (u64)(x >> 64);
    u64 carry = (u64)(((u128)x0 * m.r0) >> 64);
    u128 t = (u128)x0 * m.r1;
    u64 tmp1 = (u64)t + carry, tmp3 = (u64)(t >> 64) + (tmp1 < carry);
    t = (u128)x1 * m.r0;
    u64 tmp1b = tmp1 + (u64)t;
    carry = (u64)(t >> 64) + (tmp1b < tmp1);
    u64 r = x0 - (x1 * m.r1 + tmp3 + carry) * m.q;
    while (r >= m.q) r -= m.q;
    return r;
  }

  // negacyclic NTT, natural -> bit-reversed, canonical output
  void ntt(uint32_t i, u64 *x) const {
    const HostPrime &m = pm[i];
    const u64 q = m.q, q2 = 2 * q;
    for (uint32_t mm = 1, gap = N >> 1; mm < N; mm <<= 1, gap >>= 1)
      for (uint32_t g = 0; g < mm; g++) {
        const u64 w = m.rp[mm + g], ws = m.rps[mm + g];
        u64 *a = x + 2 * (size_t)g * gap, *b = a + gap;
        for (uint32_t j = 0; j < gap; j++) {
          u64 X = a[j];
          X -= (X >= q2) ? q2 : 0;
          u64 T = mul_shoup_lazy(b[j], w, ws, q);
          a[j] = X + T;
          b[j] = X + q2 - T;
        }
      }
    for (uint32_t j = 0; j < N; j++) {
      u64 v = x[j];
      v -= (v >= q2) ? q2 : 0;
      v -= (v >= q) ? q : 0;
      x[j] = v;
    }
  }
  void intt(uint32_t i, u64 *x) const {
    const HostPrime &m = pm[i];
    const u64 q = m.q, q2 = 2 * q;
    for (uint32_t mm = N >> 1, gap = 1; mm >= 1; mm >>= 1, gap <<= 1)
      for (uint32_t g = 0; g < mm; g++) {
        const u64 w = m.irp[mm + g], ws = m.irps[mm + g];
        u64 *a = x + 2 * (size_t)g * gap, *b = a + gap;
        for (uint32_t j = 0; j < gap; j++) {
          u64 X = a[j], Y = b[j], S = X + Y;
          a[j] = S - ((S >= q2) ? q2 : 0);
          b[j] = mul_shoup_lazy(X + q2 - Y, w, ws, q);
        }
      }
    for (uint32_t j = 0; j < N; j++) {
      u64 v = mul_shoup_lazy(x[j], m.ninv, m.ninv_s, q);
      x[j] = v >= q ? v - q : v;
    }
  }

  // residues of an integer-valued double of any magnitude: v = m * 2^e exactly (53-bit m), so
  // v mod q = (m mod q) * (2^e mod q) — what SEAL's multi-precision encode path computes
  void residues_of(double v, uint32_t limbs, u64 *out, size_t stride) const {
    const bool neg = std::signbit(v);
    const double a = std::fabs(v);
    int e = 0;
    u64 mant;
    if (a < 9007199254740992.0) { mant = (u64)a; }  // < 2^53: exact
    else {
      double fr = std::frexp(a, &e); // a = fr * 2^e, fr in [0.5,1)
      mant = (u64)std::ldexp(fr, 53);
      e -= 53;
    }
    for (uint32_t i = 0; i < limbs; i++) {
      const u64 q = primes[i];
      u64 r = mant % q;
      if (e > 0) r = evah::mulmod(r, e < (int)pow2_[i].size() ? pow2_[i][e] : evah::powmod(2, (u64)e, q), q);
      out[(size_t)i * stride] = (neg && r) ? q - r : r;
    }
  }

  // ---- CKKS encoder.  values: N/2 slots (already replicated by the caller).
  // Coefficient-form residues [limbs][N]; the forward NTT is done by the caller (device or host).
  // Floating-point operation order is SEAL 3.6's (CKKSEncoder::encode_internal reached from
  // /root/reference/eva/seal/seal_executor.h:242): Gentleman-Sande stages over the sequentially
  // stored inverse roots, and the factor scale/N applied INSIDE the last stage — sums are scaled,
  // differences are multiplied by the pre-scaled root — so the rounded coefficients are SEAL's.
  static std::complex<double> cmul(const std::complex<double> &a, const std::complex<double> &b) {
    // four rounded products, one rounded difference and sum (no fused multiply-add)
    const double p = a.real() * b.real(), q = a.imag() * b.imag();
    const double r = a.real() * b.imag(), t = a.imag() * b.real();
    return {p - q, r + t};
  }
  void encode_coeff(const double *values, double scale, uint32_t limbs, u64 *out) const {
    const uint32_t slots = N >> 1;
    std::vector<std::complex<double>> c(N);
    for (uint32_t i = 0; i < slots; i++) {
      c[slot_map_[i]] = std::complex<double>(values[i], 0.0);
      c[slot_map_[slots + i]] = std::complex<double>(values[i], -0.0); // conj of a real value
    }
    const double fix = scale / (double)N;
    size_t next_root = 1; // inv_seq_[1..N-1] in the order the stages consume them
    uint32_t gap = 1;
    for (uint32_t groups = N >> 1; groups > 1; groups >>= 1, gap <<= 1)
      for (uint32_t g = 0; g < groups; g++) {
        const std::complex<double> w = inv_seq_[next_root++];
        std::complex<double> *lo = c.data() + 2 * (size_t)g * gap, *hi = lo + gap;
        for (uint32_t j = 0; j < gap; j++) {
          const std::complex<double> u = lo[j], v = hi[j];
          lo[j] = u + v;
          hi[j] = cmul(u - v, w);
        }
      }
    { // final stage: one group, gap = N/2, scaling folded in
      const std::complex<double> w = inv_seq_[next_root], ws(w.real() * fix, w.imag() * fix);
      std::complex<double> *lo = c.data(), *hi = lo + gap;
      for (uint32_t j = 0; j < gap; j++) {
        const std::complex<double> u = lo[j], v = hi[j], s = u + v;
        lo[j] = std::complex<double>(s.real() * fix, s.imag() * fix);
        hi[j] = cmul(u - v, ws);
      }
    }
    double max_coeff = 0;
    for (uint32_t j = 0; j < N; j++) max_coeff = std::max(max_coeff, std::fabs(c[j].real()));
    int bitcount = (int)std::ceil(std::log2(std::max(max_coeff, 1.0))) + 1;
    if (bitcount >= total_bits[limbs]) throw std::invalid_argument("encoded values are too large");
    for (uint32_t j = 0; j < N; j++) residues_of(std::round(c[j].real()), limbs, out + j, N);
  }
  // residues of round(c*scale) per limb: the encoding of a uniform constant (every NTT slot)
  void encode_uniform(double value, double scale, uint32_t limbs, u64 *out) const {
    double v = std::round(value * scale);
    int bitcount = (int)std::ceil(std::log2(std::max(std::fabs(v), 1.0))) + 1;
    if (bitcount >= total_bits[limbs]) throw std::invalid_argument("encoded values are too large");
    residues_of(v, limbs, out, 1);
  }
  // coefficient-form plaintext [limbs][N] (already INTT'd) -> N/2 slot values
  void decode_coeff(const u64 *coeff, uint32_t limbs, double scale, std::vector<double> &out) const {
    std::vector<std::complex<double>> c(N);
    // mixed-radix (Garner) composition per coefficient, exact multiword compare against Q/2
    std::vector<std::vector<u64>> prefix(limbs); // prefix[i] = q_0...q_{i-1} as multiword
    prefix[0] = {1};
    for (uint32_t i = 1; i < limbs; i++) prefix[i] = mul_small(prefix[i - 1], primes[i - 1]);
    std::vector<u64> Q = mul_small(prefix[limbs - 1], primes[limbs - 1]);
    std::vector<u64> halfQ = shr1(Q);
    // inv_prefix[i] = (q_0...q_{i-1})^-1 mod q_i ; pre_mod[i][j] = q_0..q_{j-1} mod q_i
    std::vector<u64> inv_prefix(limbs, 1);
    std::vector<std::vector<u64>> pre_mod(limbs);
    for (uint32_t i = 0; i < limbs; i++) {
      u64 acc = 1 % primes[i];
      pre_mod[i].resize(i + 1);
      for (uint32_t j = 0; j < i; j++) {
        pre_mod[i][j] = acc;
        acc = evah::mulmod(acc, primes[j] % primes[i], primes[i]);
      }
      pre_mod[i][i] = acc;
      inv_prefix[i] = evah::invmod(acc, primes[i]);
    }
    std::vector<u64> v(limbs), x;
    const double inv_scale = 1.0 / scale, two_pow_64 = std::pow(2.0, 64);
    for (uint32_t j = 0; j < N; j++) {
      for (uint32_t i = 0; i < limbs; i++) {
        u64 qi = primes[i], acc = 0;
        for (uint32_t t = 0; t < i; t++) acc = evah::addmod(acc, evah::mulmod(v[t] % qi, pre_mod[i][t], qi), qi);
        u64 r = coeff[(size_t)i * N + j];
        v[i] = evah::mulmod(evah::submod(r, acc, qi), inv_prefix[i], qi);
      }
      x.assign(Q.size() + 1, 0);
      for (uint32_t i = 0; i < limbs; i++) add_mul(x, prefix[i], v[i]);
      x.resize(Q.size());
      // SEAL 3.6 CKKSEncoder::decode_internal: the base-2^64 words of the composed coefficient go into
      // ONE double, least significant first, with 1/scale folded into the running power of 2^64; a
      // coefficient above Q/2 is negative and is accumulated as signed per-word differences against the
      // words of Q.  `limbs` words per coefficient (SEAL's coeff_modulus_size), high ones zero.
      const bool negative = cmp(x, halfQ) > 0; // x >= upper_half_threshold = (Q + 1) / 2
      double acc = 0.0, scaled = inv_scale;
      for (uint32_t w = 0; w < limbs; w++, scaled *= two_pow_64) {
        const u64 xw = w < x.size() ? x[w] : 0, qw = w < Q.size() ? Q[w] : 0;
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
      c[j] = acc;
    }
    // forward special FFT (Cooley-Tukey, zeta^br(m+g))
    for (uint32_t mm = 1, gap = N >> 1; mm < N; mm <<= 1, gap >>= 1)
      for (uint32_t g = 0; g < mm; g++) {
        const std::complex<double> w = roots_[mm + g];
        std::complex<double> *a = c.data() + 2 * (size_t)g * gap, *b = a + gap;
        for (uint32_t jj = 0; jj < gap; jj++) {
          std::complex<double> u = a[jj], t = b[jj] * w;
          a[jj] = u + t;
          b[jj] = u - t;
        }
      }
    out.resize(N >> 1);
    for (uint32_t i = 0; i < (N >> 1); i++) out[i] = c[slot_map_[i]].real();
  }

  // ---- sampling
  void sample_ternary(SecureRng &rng, std::vector<int8_t> &out) const {
    out.resize(N);
    std::uniform_int_distribution<int> d(-1, 1);
    for (auto &v : out) v = (int8_t)d(rng);
  }
  // centered binomial, 21 + 21 bits: sigma ~ 3.24 (SEAL sample_poly_cbd)
  void sample_error(SecureRng &rng, std::vector<int8_t> &out) const {
    out.resize(N);
    for (auto &v : out) {
      u64 r = rng();
      v = (int8_t)(__builtin_popcountll(r & 0x1FFFFF) - __builtin_popcountll((r >> 21) & 0x1FFFFF));
    }
  }
  void small_to_ntt(const std::vector<int8_t> &s, uint32_t prime_idx, u64 *out) const {
    u64 q = primes[prime_idx];
    for (uint32_t j = 0; j < N; j++) out[j] = s[j] < 0 ? q - (u64)(-s[j]) : (u64)s[j];
    ntt(prime_idx, out);
  }
  void sample_uniform(SecureRng &rng, uint32_t prime_idx, u64 *out) const {
    u64 q = primes[prime_idx];
    u64 lim = ~(u64)0 - (~(u64)0 % q) - 1; // rejection bound
    for (uint32_t j = 0; j < N; j++) {
      u64 r;
      do r = rng(); while (r > lim);
      out[j] = r % q;
    }
  }

private:
  std::vector<std::vector<u64>> pow2_;
  std::vector<uint32_t> slot_map_;
  std::vector<std::complex<double>> roots_;   // roots_[m+g] = zeta^br(m+g), zeta = exp(2 pi i / 2N)
  std::vector<std::complex<double>> inv_seq_; // inverse-transform roots in consumption order

  void init_encoder() {
    const uint32_t slots = N >> 1, m = 2 * N;
    slot_map_.resize(N);
    u64 pos = 1;
    for (uint32_t i = 0; i < slots; i++) {
      slot_map_[i] = evah::bitrev((uint32_t)((pos - 1) >> 1), logN);
      slot_map_[slots + i] = evah::bitrev((uint32_t)((m - pos - 1) >> 1), logN);
      pos = (pos * 3) & (m - 1);
    }
    evah::CkksRoots r = evah::ckks_roots(N); // SEAL ComplexRoots doubles (hostmath.h)
    roots_ = std::move(r.fwd);
    inv_seq_ = std::move(r.inv_seq);
  }

  // ---- tiny multiword helpers (little-endian u64 words)
  static std::vector<u64> mul_small(const std::vector<u64> &a, u64 b) {
    std::vector<u64> r(a.size());
    u64 carry = 0;
    for (size_t i = 0; i < a.size(); i++) {
      u128 t = (u128)a[i] * b + carry;
      r[i] = (u64)t;
      carry = (u64)(t >> 64);
    }
    if (carry) r.push_back(carry);
    return r;
  }
  static void add_mul(std::vector<u64> &acc, const std::vector<u64> &a, u64 b) { // acc += a*b
    u64 carry = 0;
    size_t i = 0;
    for (; i < a.size(); i++) {
      u128 t = (u128)a[i] * b + acc[i] + carry;
      acc[i] = (u64)t;
      carry = (u64)(t >> 64);
    }
    for (; carry && i < acc.size(); i++) {
      u128 t = (u128)acc[i] + carry;
      acc[i] = (u64)t;
      carry = (u64)(t >> 64);
    }
  }
  static std::vector<u64> shr1(const std::vector<u64> &a) {
    std::vector<u64> r(a.size());
    for (size_t i = 0; i < a.size(); i++) r[i] = (a[i] >> 1) | (i + 1 < a.size() ? a[i + 1] << 63 : 0);
    return r;
  }
  static int cmp(const std::vector<u64> &a, const std::vector<u64> &b) {
    for (size_t i = std::max(a.size(), b.size()); i-- > 0;) {
      u64 x = i < a.size() ? a[i] : 0, y = i < b.size() ? b[i] : 0;
      if (x != y) return x > y ? 1 : -1;
    }
    return 0;
  }
  static std::vector<u64> sub(const std::vector<u64> &a, const std::vector<u64> &b) { // a - b, a >= b
    std::vector<u64> r(a.size());
    u64 borrow = 0;
    for (size_t i = 0; i < a.size(); i++) {
      u64 y = i < b.size() ? b[i] : 0;
      u128 t = (u128)a[i] - y - borrow;
      r[i] = (u64)t;
      borrow = (t >> 64) ? 1 : 0;
    }
    return r;
  }
  static double to_double(const std::vector<u64> &a) {
    double d = 0;
    for (size_t i = a.size(); i-- > 0;) d = d * 18446744073709551616.0 + (double)a[i];
    return d;
  }
};

// Zeroes secret-stream draws (error polynomials) once they are used.  The stores go through a volatile pointer: the
// vectors are destroyed right afterwards, and a plain std::fill would be a dead store the compiler may remove.
inline void wipe(std::vector<int8_t> &v) {
  volatile int8_t *p = v.data();
  for (size_t i = 0, n = v.size(); i < n; i++) p[i] = 0;
}

// the same for randomness keys and other secret bytes
inline void wipe_bytes(void *p, size_t n) {
  volatile unsigned char *v = static_cast<volatile unsigned char *>(p);
  while (n--) *v++ = 0;
}
// the next 32-byte key of a stream: 4 words, little-endian, as the seeds of DESIGN.md 1.3 are drawn
inline std::array<uint8_t, 32> draw_key32(SecureRng &rng) {
  std::array<uint8_t, 32> k;
  for (int w = 0; w < 4; w++) {
    const uint64_t x = rng();
    std::memcpy(k.data() + 8 * w, &x, 8);
  }
  return k;
}
// (u, e0, e1) of a randomness key as int8 [3][N]
inline std::vector<int8_t> sampled_small3(const std::array<uint8_t, 32> &rk, uint32_t N) {
  std::vector<int8_t> small((size_t)3 * N);
  for (uint32_t p = 0; p < 3; p++) sampled_small(rk.data(), p, N, small.data() + (size_t)p * N);
  return small;
}

// Key material in the layout libeva_hip.so expects.
struct SwitchKey {
  uint32_t n_digits = 0;
  std::vector<u64> data; // [digit][2][k][N], NTT form; empty while the key is kept in its compressed form
  // the compressed form: c1 of digit J is public and uniform, so it is kept as the 32-byte seed it is
  // expanded from — row i = seeded_limb(seed_J, i, q_i, N) — beside c0.  Half the words in memory, in files and over PCIe.
  // [digit][k][N].  Empty while a key generated in place (generate_keys(..., device_keygen, device_sampling), DESIGN.md
  // 1.8) has its c0 only on the device: c0_words() fetches it on first need through `source` and keeps it
  mutable std::vector<u64> c0;
  std::vector<uint8_t> seeds; // [digit][32]
  std::function<void(std::vector<u64> &)> source; // fills c0 from where the key lives (evah_key_download_c0)
  bool compressed() const { return !seeds.empty(); }
  // the one way to read c0: a key generated in place becomes an ordinary compressed key at its first call
  const std::vector<u64> &c0_words() const {
    if (c0.empty() && source) source(c0);
    return c0;
  }
  // words of c0 / data held on the host right now
  size_t host_words() const { return c0.size() + data.size(); }
  // the full words [digit][2][k][N]: `data`, or materialised into `tmp` (never stored back: a compressed key stays compressed)
  const std::vector<u64> &words(const HostContext &cx, std::vector<u64> &tmp) const {
    if (!compressed()) return data;
    const size_t poly = (size_t)cx.k * cx.N;
    const std::vector<u64> &c0 = c0_words();
    if (c0.size() != n_digits * poly || seeds.size() != (size_t)32 * n_digits) throw std::runtime_error("compressed key: c0 or its seeds do not match the shape");
    tmp.resize((size_t)n_digits * 2 * poly);
    for (uint32_t J = 0; J < n_digits; J++) {
      u64 *d = tmp.data() + (size_t)J * 2 * poly;
      std::copy(c0.begin() + (size_t)J * poly, c0.begin() + (size_t)(J + 1) * poly, d);
      for (uint32_t i = 0; i < cx.k; i++) seeded_limb(seeds.data() + (size_t)32 * J, i, cx.primes[i], cx.N, (uint64_t *)(d + poly + (size_t)i * cx.N));
    }
    return tmp;
  }
};

struct SecretKey {
  std::vector<int8_t> s;       // ternary coefficients
  std::vector<u64> s_ntt;      // [k][N]
};
struct PublicKey {
  std::vector<u64> data; // [2][k][N], NTT form: (-(a s + e), a)
};

class KeyGenerator {
public:
  const HostContext &cx;
  // two independent ChaCha20 streams: `secret` draws the secret key and the error polynomials,
  // `pub` the uniform polynomials that are published as part of every key — nothing an observer of
  // the keys sees comes from the stream that produced the secret.  seed == 0: both keyed from the
  // OS (getrandom); seed != 0 is the reproducible test hook (csprng.h).
  std::unique_ptr<SecureRng> secret, pub;
  SecretKey sk;
  // The sampled mode (generate_keys(..., device_sampling)): every polynomial has a 32-byte key of its own.
  // Secret stream, in order: rk_s, ek_pk, then one error key per digit of every evaluation key in key order; public stream:
  // seed_pk, then one seed per digit — what draw_seeded_digit draws.  s = sampled_small(rk_s, 0), the public key is
  // (-(a s + NTT(e)), a) with a_i = seeded_limb(seed_pk, i) and e = sampled_small(ek_pk, 1), digit J's error is
  // sampled_small(ek_J, 1).  The device draws the same polynomials from the same keys (evah_keygen_public, evah_keygen_set).
  const bool sampled;
  std::array<uint8_t, 32> ek_pk{}, seed_pk{};
  // test hook, filled in the sampled mode when seed != 0 only: the keys the secret stream gave
  struct Randomness {
    std::vector<uint8_t> rk_s, ek_pk;
    std::map<uint32_t, std::vector<uint8_t>> ekeys; // 0: the relinearization key's [digits][32], Galois element: that key's
  } kept;
  const bool keep;
  // common_seed32: `pub` is keyed with these 32 bytes instead — the stream every party of a collective
  // key generation draws the same seeds from; the draw order is untouched
  KeyGenerator(const HostContext &c, uint64_t seed, bool sampled_ = false, const uint8_t *common_seed32 = nullptr)
      : cx(c), sampled(sampled_), keep(sampled_ && seed != 0) {
    if (seed) {
      secret = std::make_unique<SecureRng>(seed, 1);
      pub = std::make_unique<SecureRng>(seed, 2);
    } else {
      secret = std::make_unique<SecureRng>();
      pub = std::make_unique<SecureRng>();
    }
    if (common_seed32) pub = std::make_unique<SecureRng>(SecureRng::CommonSeed{common_seed32});
    if (sampled) {
      std::array<uint8_t, 32> rk_s = draw_key32(*secret);
      ek_pk = draw_key32(*secret);
      seed_pk = draw_key32(*pub);
      sk.s.resize(cx.N);
      sampled_small(rk_s.data(), 0, cx.N, sk.s.data());
      if (keep) {
        kept.rk_s.assign(rk_s.begin(), rk_s.end());
        kept.ek_pk.assign(ek_pk.begin(), ek_pk.end());
      }
      wipe_bytes(rk_s.data(), 32);
    } else {
      cx.sample_ternary(*secret, sk.s);
    }
    sk.s_ntt.resize((size_t)cx.k * cx.N);
    for (uint32_t i = 0; i < cx.k; i++) cx.small_to_ntt(sk.s, i, sk.s_ntt.data() + (size_t)i * cx.N);
  }
  ~KeyGenerator() { wipe_bytes(ek_pk.data(), 32); }
  PublicKey public_key() {
    PublicKey pk;
    pk.data.resize((size_t)2 * cx.k * cx.N);
    u64 *c0 = pk.data.data(), *c1 = c0 + (size_t)cx.k * cx.N;
    if (sampled) {
      for (uint32_t i = 0; i < cx.k; i++) seeded_limb(seed_pk.data(), i, cx.primes[i], cx.N, (uint64_t *)(c1 + (size_t)i * cx.N));
      std::vector<int8_t> e(cx.N);
      sampled_small(ek_pk.data(), 1, cx.N, e.data());
      zero_symmetric(c0, c1, e);
      wipe(e);
    } else {
      encrypt_zero_symmetric(c0, c1);
    }
    return pk;
  }
  // What one digit of a seed-compressed key draws, and in which order — the one place that says so, for the host
  // generator below and for the device's (client.h generate_keys(..., device_keygen)): 4 words of the
  // public stream, which are the 32-byte seed of c1, then one error polynomial of the secret stream
  void draw_seeded_digit(uint8_t *seed32, std::vector<int8_t> &e) {
    for (int w = 0; w < 4; w++) {
      const u64 r = (*pub)();
      std::memcpy(seed32 + 8 * w, &r, 8);
    }
    cx.sample_error(*secret, e);
  }
  // The same for the sampled mode, and as much the one place that says so for the host twin below and for the device's
  // set (client.h): the same 4 words of the public stream, then 4 words of the secret stream — the 32-byte key the
  // digit's error is expanded from, sampled_small(ekey32, 1)
  void draw_sampled_digit(uint8_t *seed32, uint8_t *ekey32) {
    for (int w = 0; w < 4; w++) {
      const u64 r = (*pub)();
      std::memcpy(seed32 + 8 * w, &r, 8);
    }
    for (int w = 0; w < 4; w++) {
      const u64 r = (*secret)();
      std::memcpy(ekey32 + 8 * w, &r, 8);
    }
  }
  // test hook: remember the error keys [digits][32] of key `id` (0: relinearization, else the Galois element)
  void keep_ekeys(uint32_t id, const uint8_t *ekeys, uint32_t digits) {
    if (keep) kept.ekeys[id].assign(ekeys, ekeys + (size_t)32 * digits);
  }
  // key-switch key from s' (NTT form over all k primes) to s: digit J carries P * s' in limb J.
  // seeded: c1 of every digit is the expansion of a 32-byte seed — 4 words of the public stream in place
  // of its k N rejection-sampled draws — and the key is returned as c0 + seeds
  // sampled mode: always seeded, the error of digit J expanded from its 32-byte key; id names the key for the test hook
  SwitchKey switch_key(const std::vector<u64> &sprime_ntt, bool seeded = false, uint32_t id = 0) {
    const uint32_t N = cx.N, k = cx.k, D = k - 1;
    seeded = seeded || sampled;
    std::vector<uint8_t> ekeys(sampled ? (size_t)32 * D : 0);
    SwitchKey key;
    key.n_digits = D;
    if (seeded) {
      key.c0.resize((size_t)D * k * N);
      key.seeds.resize((size_t)32 * D);
    } else {
      key.data.resize((size_t)D * 2 * k * N);
    }
    const u64 P = cx.primes[k - 1];
    std::vector<u64> a;
    std::vector<int8_t> e;
    for (uint32_t J = 0; J < D; J++) {
      u64 *c0, *c1;
      if (seeded) {
        uint8_t *seed = key.seeds.data() + (size_t)32 * J;
        if (sampled) {
          draw_sampled_digit(seed, ekeys.data() + (size_t)32 * J);
          e.resize(N);
          sampled_small(ekeys.data() + (size_t)32 * J, 1, N, e.data());
        } else {
          draw_seeded_digit(seed, e);
        }
        a.resize((size_t)k * N);
        for (uint32_t i = 0; i < k; i++) seeded_limb(seed, i, cx.primes[i], N, (uint64_t *)(a.data() + (size_t)i * N));
        c0 = key.c0.data() + (size_t)J * k * N;
        c1 = a.data();
        zero_symmetric(c0, c1, e);
        wipe(e);
      } else {
        c0 = key.data.data() + (size_t)J * 2 * k * N;
        c1 = c0 + (size_t)k * N;
        encrypt_zero_symmetric(c0, c1);
      }
      const u64 q = cx.primes[J], f = P % q;
      u64 *dst = c0 + (size_t)J * N;
      const u64 *sp = sprime_ntt.data() + (size_t)J * N;
      for (uint32_t j = 0; j < N; j++) dst[j] = evah::addmod(dst[j], cx.mulm(sp[j], f, J), q);
    }
    if (sampled) {
      keep_ekeys(id, ekeys.data(), D);
      wipe_bytes(ekeys.data(), ekeys.size());
    }
    return key;
  }
  SwitchKey relin_key(bool seeded = false) {
    std::vector<u64> s2((size_t)cx.k * cx.N);
    for (uint32_t i = 0; i < cx.k; i++)
      for (uint32_t j = 0; j < cx.N; j++) {
        u64 v = sk.s_ntt[(size_t)i * cx.N + j];
        s2[(size_t)i * cx.N + j] = cx.mulm(v, v, i);
      }
    return switch_key(s2, seeded);
  }
  SwitchKey galois_key(uint32_t elt, bool seeded = false) {
    // s(X^elt) in NTT form = permutation of s_ntt (same table as the device uses)
    std::vector<u64> sp((size_t)cx.k * cx.N);
    for (uint32_t j = 0; j < cx.N; j++) {
      uint32_t reversed = evah::bitrev(cx.N + j, cx.logN + 1);
      u64 raw = (((u64)elt * reversed) >> 1) & (u64)(cx.N - 1);
      uint32_t src = evah::bitrev((uint32_t)raw, cx.logN);
      for (uint32_t i = 0; i < cx.k; i++) sp[(size_t)i * cx.N + j] = sk.s_ntt[(size_t)i * cx.N + src];
    }
    return switch_key(sp, seeded, elt);
  }

private:
  // (c0, c1) = (-(a s + e), a) over all k primes, NTT form, with fresh e (secret stream) and a (public stream)
  void encrypt_zero_symmetric(u64 *c0, u64 *c1) {
    std::vector<int8_t> e;
    cx.sample_error(*secret, e);
    for (uint32_t i = 0; i < cx.k; i++) cx.sample_uniform(*pub, i, c1 + (size_t)i * cx.N);
    zero_symmetric(c0, c1, e);
  }
  // c0 = -(a s + e) for a given in c1 and e given
  void zero_symmetric(u64 *c0, const u64 *c1, const std::vector<int8_t> &e) {
    const uint32_t N = cx.N;
    std::vector<u64> en(N);
    for (uint32_t i = 0; i < cx.k; i++) {
      const u64 q = cx.primes[i];
      const u64 *a = c1 + (size_t)i * N;
      u64 *b = c0 + (size_t)i * N;
      cx.small_to_ntt(e, i, en.data());
      const u64 *s = sk.s_ntt.data() + (size_t)i * N;
      for (uint32_t j = 0; j < N; j++) b[j] = evah::negmod(evah::addmod(cx.mulm(a[j], s[j], i), en[j], q), q);
    }
  }
};

// Host ciphertext / plaintext values (what encrypt() hands to execute() and execute() to decrypt())
// Ciphertext words live in pinned host memory when the device library can provide it
// (evah_host_alloc): they are what execute() uploads and downloads, and DMA from pinned pages runs
// at PCIe rate.  Without a device the allocator is plain operator new.
template <class T> struct HostAlloc {
  using value_type = T;
  HostAlloc() = default;
  template <class U> HostAlloc(const HostAlloc<U> &) {}
  T *allocate(size_t n) {
    // 64-byte header in front of the data remembers where the block came from
    const size_t bytes = n * sizeof(T) + 64;
    char *base = static_cast<char *>(evah_host_alloc(bytes));
    const bool pinned = base != nullptr;
    if (!base) base = static_cast<char *>(::operator new(bytes));
    *reinterpret_cast<uint64_t *>(base) = pinned ? 0x50494e4eull : 0x48454150ull;
    return reinterpret_cast<T *>(base + 64);
  }
  void deallocate(T *p, size_t) {
    char *base = reinterpret_cast<char *>(p) - 64;
    if (*reinterpret_cast<uint64_t *>(base) == 0x50494e4eull) evah_host_free(base);
    else ::operator delete(base);
  }
  // resize() leaves new words uninitialised (every user overwrites them: downloads, encrypt): a
  // value-initialising resize of a 256-instance output batch would memset 134 MB on the host
  template <class U, class... A> void construct(U *p, A &&...a) {
    if constexpr (sizeof...(A) == 0) ::new ((void *)p) U;
    else ::new ((void *)p) U(std::forward<A>(a)...);
  }
  template <class U> bool operator==(const HostAlloc<U> &) const { return true; }
  template <class U> bool operator!=(const HostAlloc<U> &) const { return false; }
};
using CipherWords = std::vector<u64, HostAlloc<u64>>;
// A ciphertext value of a valuation.  It may live on the host (data), on the device (dev: a handle
// of a device context, executor.h) or both: SURVEY.md 8(b) keeps the reference's SEALValuation
// opaque so that it "may hold device handles", and encrypt -> execute -> decrypt then never moves a
// ciphertext over PCIe.  The host words are filled on demand (words(): a download) — by get(),
// save(), a context on another device, or the host-only code paths.
struct DeviceResident;
// A symmetric ciphertext sent as c0 plus the seed of c1 = a: c1's words follow from (seed, limb)
// alone (seeded_limb, csprng.h), so the value costs half the words of a full ciphertext on the wire and over PCIe
struct SeededForm {
  std::array<uint8_t, 32> seed{};
  CipherWords c0;          // [limbs][N]; empty when the value is device-resident (the handle holds c0)
  std::vector<u64> primes; // the chain c1 is reduced by (limb i -> primes[i]), so words() needs no context
  uint32_t N = 0;
};
struct HostCipher {
  uint32_t size = 0, limbs = 0;
  double scale = 1.0;
  mutable CipherWords data; // [size][limbs][N]; empty while the value lives only on the device or in its seeded form
  std::shared_ptr<DeviceResident> dev;
  mutable bool words_checked = false; // every word < its prime: verified (values from files / Python) or by construction
  std::shared_ptr<const SeededForm> seeded; // set by HipSecret::encrypt (and load()); never by execute()
};
struct HostPlain {
  uint32_t limbs = 0;
  double scale = 1.0;
  std::vector<u64> data; // [limbs][N], NTT form
  mutable bool words_checked = false;
};

// Secret-key encryption of an NTT-form plaintext at its limbs: c1 = a expanded from `seed`,
// c0 = m - (a s + NTT(e)) — the sign convention of KeyGenerator::encrypt_zero_symmetric; no special prime, no
// mod-down.  The value is returned in its seeded form (c0 + seed); words() materialises c1.
inline HostCipher encrypt_symmetric(const HostContext &cx, const SecretKey &sk, const HostPlain &pt, const std::vector<int8_t> &e,
                                    const std::array<uint8_t, 32> &seed) {
  const uint32_t N = cx.N, l = pt.limbs;
  if (l < 1 || l > cx.k - 1) throw std::invalid_argument("plaintext level is not valid for encryption");
  auto sf = std::make_shared<SeededForm>();
  sf->seed = seed;
  sf->N = N;
  sf->primes.assign(cx.primes.begin(), cx.primes.begin() + l);
  sf->c0.resize((size_t)l * N);
  std::vector<u64> a(N), en(N);
  for (uint32_t i = 0; i < l; i++) {
    const u64 q = cx.primes[i];
    seeded_limb(seed.data(), i, q, N, (uint64_t *)a.data());
    cx.small_to_ntt(e, i, en.data());
    const u64 *m = pt.data.data() + (size_t)i * N, *s = sk.s_ntt.data() + (size_t)i * N;
    u64 *c0 = sf->c0.data() + (size_t)i * N;
    for (uint32_t j = 0; j < N; j++) c0[j] = evah::submod(m[j], evah::addmod(cx.mulm(a[j], s[j], i), en[j], q), q);
  }
  std::fill(en.begin(), en.end(), 0);
  HostCipher out;
  out.size = 2;
  out.limbs = l;
  out.scale = pt.scale;
  out.words_checked = true;
  out.seeded = std::move(sf);
  return out;
}
// the full words [2][l][N] of a seeded value from its host form
inline void materialise_seeded(const SeededForm &sf, uint32_t limbs, CipherWords &out) {
  const size_t each = (size_t)limbs * sf.N;
  if (sf.c0.size() != each || sf.primes.size() < limbs) throw std::runtime_error("seeded ciphertext: c0 or its primes do not match the shape");
  out.resize(2 * each);
  std::copy(sf.c0.begin(), sf.c0.end(), out.begin());
  for (uint32_t i = 0; i < limbs; i++) seeded_limb(sf.seed.data(), i, sf.primes[i], sf.N, (uint64_t *)(out.data() + each + (size_t)i * sf.N));
}

// Public-key encryption of an NTT-form plaintext at `limbs` data limbs (A.10): encrypt zero one
// level up (limbs+1 primes), divide-and-round by that extra prime, add the plaintext to c0.
// The randomness is the caller's: u ternary, e0 and e1 error polynomials, N coefficients each.
inline HostCipher encrypt(const HostContext &cx, const PublicKey &pk, const HostPlain &pt, const std::vector<int8_t> &u,
                          const std::vector<int8_t> &e0, const std::vector<int8_t> &e1) {
  const uint32_t N = cx.N, l = pt.limbs, up = l + 1;
  if (up > cx.k) throw std::invalid_argument("plaintext level is not valid for encryption");
  if (u.size() != N || e0.size() != N || e1.size() != N) throw std::invalid_argument("encryption randomness must be three polynomials of N coefficients");
  std::vector<u64> c((size_t)2 * up * N), un(N), en(N);
  for (uint32_t i = 0; i < up; i++) {
    const u64 q = cx.primes[i];
    cx.small_to_ntt(u, i, un.data());
    for (uint32_t K = 0; K < 2; K++) {
      cx.small_to_ntt(K ? e1 : e0, i, en.data());
      const u64 *p = pk.data.data() + ((size_t)K * cx.k + i) * N;
      u64 *dst = c.data() + ((size_t)K * up + i) * N;
      for (uint32_t j = 0; j < N; j++) dst[j] = evah::addmod(cx.mulm(p[j], un[j], i), en[j], q);
    }
  }
  // divide and round by the last of the `up` primes (same rule as rescale, A.5)
  HostCipher out;
  out.size = 2;
  out.limbs = l;
  out.scale = pt.scale;
  out.data.resize((size_t)2 * l * N);
  const uint32_t last = up - 1;
  const u64 ql = cx.primes[last], half = ql >> 1;
  std::vector<u64> t(N), w(N);
  for (uint32_t K = 0; K < 2; K++) {
    std::copy_n(c.data() + ((size_t)K * up + last) * N, N, t.data());
    cx.intt(last, t.data());
    for (uint32_t j = 0; j < N; j++) t[j] = evah::addmod(t[j], half, ql);
    for (uint32_t i = 0; i < l; i++) {
      const u64 q = cx.primes[i], hq = half % q, inv = evah::invmod(ql % q, q);
      for (uint32_t j = 0; j < N; j++) w[j] = evah::submod(t[j] % q, hq, q);
      cx.ntt(i, w.data());
      const u64 *src = c.data() + ((size_t)K * up + i) * N;
      u64 *dst = out.data.data() + ((size_t)K * l + i) * N;
      for (uint32_t j = 0; j < N; j++) {
        u64 v = cx.mulm(evah::submod(src[j], w[j], q), inv, i);
        dst[j] = K == 0 ? evah::addmod(v, pt.data[(size_t)i * N + j], q) : v;
      }
    }
  }
  return out;
}

// the same with u, e0, e1 drawn from rng, in that order
inline HostCipher encrypt(const HostContext &cx, const PublicKey &pk, const HostPlain &pt, SecureRng &rng) {
  if (pt.limbs + 1 > cx.k) throw std::invalid_argument("plaintext level is not valid for encryption");
  std::vector<int8_t> u, e0, e1;
  cx.sample_ternary(rng, u);
  cx.sample_error(rng, e0);
  cx.sample_error(rng, e1);
  return encrypt(cx, pk, pt, u, e0, e1);
}

// m = c0 + c1 s (+ c2 s^2), NTT form -> coefficient form per limb
inline std::vector<u64> decrypt_to_coeff(const HostContext &cx, const SecretKey &sk, const HostCipher &ct) {
  const uint32_t N = cx.N, l = ct.limbs;
  std::vector<u64> m((size_t)l * N);
  for (uint32_t i = 0; i < l; i++) {
    const u64 q = cx.primes[i];
    const u64 *s = sk.s_ntt.data() + (size_t)i * N;
    u64 *dst = m.data() + (size_t)i * N;
    for (uint32_t j = 0; j < N; j++) {
      u64 acc = ct.data[((size_t)0 * l + i) * N + j], sp = s[j];
      for (uint32_t p = 1; p < ct.size; p++) {
        acc = evah::addmod(acc, cx.mulm(ct.data[((size_t)p * l + i) * N + j], sp, i), q);
        sp = cx.mulm(sp, s[j], i);
      }
      dst[j] = acc;
    }
    cx.intt(i, dst);
  }
  return m;
}

// The exponent a of a scale 2^a with a an integer; anything else is refused (the refresh's scales)
inline int pow2_exponent(double scale) {
  int e = 0;
  if (!(scale > 0) || !std::isfinite(scale) || std::frexp(scale, &e) != 0.5)
    throw std::invalid_argument("scale is not a power of two: refresh takes scales 2^a with a an integer");
  return e - 1;
}
// the shift t = a - b of a refresh from scale 2^a to scale 2^b: 0 <= t <= 62
inline uint32_t refresh_shift(double scale_in, double scale_out) {
  const int t = pow2_exponent(scale_in) - pow2_exponent(scale_out);
  if (t < 0) throw std::invalid_argument("the target scale is above the value's: refresh divides, it does not multiply");
  if (t > 62) throw std::invalid_argument("the scale ratio exceeds 2^62");
  return (uint32_t)t;
}
// Garner's constants of a level: inv_prefix[i] = (q_0..q_{i-1})^-1 mod q_i, pre_mod[i * l + j] = q_0..q_{j-1} mod q_i
struct GarnerTab {
  std::vector<u64> inv_prefix, pre_mod;
  GarnerTab(const std::vector<u64> &primes, uint32_t l) : inv_prefix(l), pre_mod((size_t)l * l) {
    for (uint32_t i = 0; i < l; i++) {
      const u64 qi = primes[i];
      u64 acc = 1 % qi;
      for (uint32_t j = 0; j < i; j++) {
        pre_mod[(size_t)i * l + j] = acc;
        acc = evah::mulmod(acc, primes[j] % qi, qi);
      }
      inv_prefix[i] = evah::invmod(acc, qi);
    }
  }
};
// One coefficient of the refresh: residues r[i] (i < l) of U in [0, Q_l) -> out[j] (j < L), the residues
// of floor((M + 2^(t-1)) / 2^t) with M = U for U <= floor(Q_l / 2), else U - Q_l (ties towards +infinity).  The steps, the
// table (hostmath.h lift_table_build) and so the words are the device kernel's (client.hip k_refresh_lift).
inline void refresh_lift_coeff(const std::vector<u64> &primes, const std::vector<u64> &tab, uint32_t l, uint32_t L, uint32_t t, const u64 *r,
                               const GarnerTab &g, u64 *v, u64 *out) {
  const evah::LiftLayout at{l, L};
  for (uint32_t i = 0; i < l; i++) { // Garner: U = sum_i v_i q_0..q_{i-1}
    const u64 qi = primes[i];
    u64 acc = 0;
    for (uint32_t j = 0; j < i; j++) acc = evah::addmod(acc, evah::mulmod(v[j] % qi, g.pre_mod[(size_t)i * l + j], qi), qi);
    v[i] = i ? evah::mulmod(evah::submod(r[i], acc, qi), g.inv_prefix[i], qi) : r[0];
  }
  bool neg = false;
  for (uint32_t i = l; i-- > 0;)
    if (v[i] != tab[at.half() + i]) { neg = v[i] > tab[at.half() + i]; break; }
  u64 w = 0;
  for (uint32_t i = 0; i < l; i++) w += v[i] * tab[at.wpre() + i];
  if (neg) w -= tab[at.qw()];
  const u64 hb = t ? (u64)1 << (t - 1) : 0, rho = t ? (w + hb) & (((u64)1 << t) - 1) : 0;
  const int64_t d = (int64_t)hb - (int64_t)rho; // |d| <= 2^61
  for (uint32_t j = 0; j < L; j++) {
    const u64 qj = primes[j];
    u64 m;
    if (j < l) {
      m = r[j];
    } else {
      m = 0;
      for (uint32_t i = 0; i < l; i++) m = evah::addmod(m, evah::mulmod(v[i] % qj, tab[at.premod() + (size_t)(j - l) * l + i], qj), qj);
    }
    if (neg) m = evah::submod(m, tab[at.qmod() + j], qj);
    if (t) {
      const u64 dm = d < 0 ? evah::negmod((u64)(-d) % qj, qj) : (u64)d % qj;
      m = evah::mulmod(evah::addmod(m, dm, qj), tab[at.inv2t() + j], qj);
    }
    out[j] = m;
  }
}
// The refresh on the host: decrypt ct (size 2 or 3, l limbs, scale 2^a), divide the integer message by
// 2^t with the rule above, and encrypt it again under sk at L limbs and scale 2^(a - t): error = sampled_small(ek, 1), c1
// from `seed`.  No decode, no floating point.  Word for word what evah_refresh_handles gives.
inline HostCipher refresh_host(const HostContext &cx, const SecretKey &sk, const HostCipher &ct, uint32_t L, uint32_t t,
                               const std::array<uint8_t, 32> &ek, const std::array<uint8_t, 32> &seed) {
  const uint32_t N = cx.N, l = ct.limbs;
  if (ct.size < 1 || ct.size > 3) throw std::invalid_argument("ciphertext size out of range");
  if (l < 1 || l > cx.k - 1 || L < 1 || L > cx.k - 1) throw std::invalid_argument("invalid limb count for this context");
  if (t > 62) throw std::invalid_argument("the scale ratio exceeds 2^62");
  if (ct.data.size() != (size_t)ct.size * l * N) throw std::invalid_argument("ciphertext words do not match its shape");
  std::vector<u64> m = decrypt_to_coeff(cx, sk, ct);
  const std::vector<u64> tab = evah::lift_table_build(cx.primes, l, L, t);
  const GarnerTab g(cx.primes, l);
  HostPlain pt;
  pt.limbs = L;
  pt.scale = std::ldexp(ct.scale, -(int)t);
  pt.data.resize((size_t)L * N);
  std::vector<u64> r(l), v(l), o(L);
  for (uint32_t n = 0; n < N; n++) {
    for (uint32_t i = 0; i < l; i++) r[i] = m[(size_t)i * N + n];
    refresh_lift_coeff(cx.primes, tab, l, L, t, r.data(), g, v.data(), o.data());
    for (uint32_t j = 0; j < L; j++) pt.data[(size_t)j * N + n] = o[j];
  }
  for (uint32_t j = 0; j < L; j++) cx.ntt(j, pt.data.data() + (size_t)j * N);
  std::vector<int8_t> e(N);
  sampled_small(ek.data(), 1, N, e.data());
  HostCipher out = encrypt_symmetric(cx, sk, pt, e, seed);
  wipe(e);
  wipe_bytes(m.data(), m.size() * sizeof(u64));
  wipe_bytes(pt.data.data(), pt.data.size() * sizeof(u64));
  return out;
}

// ---- threshold decryption: the host twins of evah_decrypt_share_handles and evah_decrypt_combine_rows
// is P 2^(sigma + 2) > Q_l ?  The flooding noise of P parties must leave the message below Q_l / 2.
inline bool flood_exceeds_modulus(const std::vector<u64> &primes, uint32_t l, uint32_t parties, uint32_t sigma) {
  unsigned __int128 Q = 1;
  for (uint32_t i = 0; i < l; i++) {
    if (Q >> 64) return false; // Q_l >= 2^64 2^29 already: above 64 2^64
    Q *= primes[i];
  }
  return ((unsigned __int128)parties << (sigma + 2)) > Q;
}
// One party's share of a size-2 ciphertext of l limbs: h[i] = c1[i] s_p[i] + NTT_i(E), E = flood_wide(fk, sigma), the
// residue of E_j under q_i being |E_j| mod q_i, negated for E_j < 0.  [l][N], canonical residues: the device's words.
inline std::vector<u64> decrypt_share_host(const HostContext &cx, const SecretKey &sk, const HostCipher &ct, uint32_t sigma,
                                           const std::array<uint8_t, 32> &fk) {
  const uint32_t N = cx.N, l = ct.limbs;
  if (ct.size != 2) throw std::invalid_argument("decryption share expects a size-2 ciphertext (relinearize first)");
  if (l < 1 || l > cx.k - 1) throw std::invalid_argument("invalid limb count for this context");
  if (ct.data.size() != (size_t)2 * l * N) throw std::invalid_argument("ciphertext words do not match its shape");
  if (sk.s_ntt.size() != (size_t)cx.k * N) throw std::invalid_argument("secret key not present");
  if (sigma < 1 || sigma > 62) throw std::invalid_argument("smudge_bits must be 1..62");
  if (flood_exceeds_modulus(cx.primes, l, 1, sigma)) throw std::invalid_argument("smudge_bits leaves no room at this level");
  std::vector<int64_t> E(N);
  flood_wide(fk.data(), sigma, N, E.data());
  std::vector<u64> h((size_t)l * N);
  for (uint32_t i = 0; i < l; i++) {
    const u64 q = cx.primes[i];
    u64 *dst = h.data() + (size_t)i * N;
    for (uint32_t j = 0; j < N; j++) {
      const u64 r = (u64)(E[j] < 0 ? -E[j] : E[j]) % q;
      dst[j] = E[j] < 0 && r ? q - r : r;
    }
    cx.ntt(i, dst);
    const u64 *c1 = ct.data.data() + ((size_t)l + i) * N, *s = sk.s_ntt.data() + (size_t)i * N;
    for (uint32_t j = 0; j < N; j++) dst[j] = evah::addmod(cx.mulm(c1[j], s[j], i), dst[j], q);
  }
  wipe_bytes(E.data(), E.size() * sizeof(int64_t));
  return h;
}
// m = c0 + sum_p h_p per limb, in coefficient form [l][N] (decrypt_to_coeff's inverse transforms): what decode_coeff
// turns into the slot values at the ciphertext's scale.  Needs no secret key.
inline std::vector<u64> combine_shares_host(const HostContext &cx, const HostCipher &ct, const std::vector<const u64 *> &shares, uint32_t sigma) {
  const uint32_t N = cx.N, l = ct.limbs;
  if (ct.size != 2) throw std::invalid_argument("decryption share expects a size-2 ciphertext (relinearize first)");
  if (l < 1 || l > cx.k - 1) throw std::invalid_argument("invalid limb count for this context");
  if (ct.data.size() != (size_t)2 * l * N) throw std::invalid_argument("ciphertext words do not match its shape");
  if (shares.empty() || shares.size() > 64) throw std::invalid_argument("the number of parties must be 1..64");
  if (sigma < 1 || sigma > 62) throw std::invalid_argument("smudge_bits must be 1..62");
  if (flood_exceeds_modulus(cx.primes, l, (uint32_t)shares.size(), sigma))
    throw std::invalid_argument("smudge_bits leaves no room at this level for this many parties");
  std::vector<u64> m(ct.data.begin(), ct.data.begin() + (size_t)l * N);
  for (uint32_t i = 0; i < l; i++) {
    const u64 q = cx.primes[i];
    u64 *dst = m.data() + (size_t)i * N;
    for (const u64 *h : shares)
      for (uint32_t j = 0; j < N; j++) dst[j] = evah::addmod(dst[j], h[(size_t)i * N + j], q);
    cx.intt(i, dst);
  }
  return m;
}

// ---- re-key to another key pair
// The key that takes ciphertexts under key pair A to key pair B of the same parameters: what B's public context installs
// and applies.  Not seed-compressible (its c1 is pkB1 u + e1, no expansion): kept, saved and sent whole.
struct RekeyKey {
  uint32_t N = 0, n_digits = 0;
  std::vector<u64> primes;
  std::vector<u64> data; // [digit][2][k][N], NTT form
};
// The host twin of evah_keygen_rekey, word for word: for digit J and prime row i
//   d[J][0][i] = pkB0_i u_J + NTT_i(e0_J) + [i == J] (P mod q_J) sA_i,   d[J][1][i] = pkB1_i u_J + NTT_i(e1_J)
// with (u_J, e0_J, e1_J) = sampled_small(rkeys[J], 0 / 1 / 2) — the zero encryption of encrypt() above under B's public
// key, at the key level and without its mod-down, plus P sA on the digit's own row.
inline std::vector<u64> rekey_keygen_host(const HostContext &cx, const SecretKey &sk, const PublicKey &pk_target, uint32_t n_digits,
                                          const std::array<uint8_t, 32> *rkeys) {
  const uint32_t N = cx.N, k = cx.k;
  if (n_digits == 0 || n_digits > k - 1) throw std::invalid_argument("invalid key digit count");
  if (pk_target.data.size() != (size_t)2 * k * N) throw std::invalid_argument("the target's public key does not match the encryption parameters");
  if (sk.s_ntt.size() != (size_t)k * N) throw std::invalid_argument("secret key not present");
  const size_t poly = (size_t)k * N;
  const u64 P = cx.primes[k - 1];
  std::vector<u64> out((size_t)n_digits * 2 * poly), un(N), en(N);
  for (uint32_t J = 0; J < n_digits; J++) {
    std::vector<int8_t> small = sampled_small3(rkeys[J], N);
    std::vector<int8_t> u(small.begin(), small.begin() + N), e(N);
    for (uint32_t i = 0; i < k; i++) {
      const u64 q = cx.primes[i];
      cx.small_to_ntt(u, i, un.data());
      for (uint32_t K = 0; K < 2; K++) {
        std::copy_n(small.begin() + (size_t)(1 + K) * N, N, e.begin());
        cx.small_to_ntt(e, i, en.data());
        const u64 *p = pk_target.data.data() + (size_t)K * poly + (size_t)i * N;
        u64 *dst = out.data() + ((size_t)2 * J + K) * poly + (size_t)i * N;
        for (uint32_t j = 0; j < N; j++) dst[j] = evah::addmod(cx.mulm(p[j], un[j], i), en[j], q);
        if (K == 0 && i == J) {
          const u64 pmod = P % q, *s = sk.s_ntt.data() + (size_t)i * N;
          for (uint32_t j = 0; j < N; j++) dst[j] = evah::addmod(dst[j], cx.mulm(s[j], pmod, i), q);
        }
      }
    }
    wipe(small);
    wipe(u);
    wipe(e);
  }
  std::fill(un.begin(), un.end(), 0);
  std::fill(en.begin(), en.end(), 0);
  return out;
}

// ---- the collective relinearization key: the host twins of evah_keygen_relin_round1 / _round2, word for
// word.  A share of either round, as it travels between the parties: round 1 [digit][2][k][N], round 2 [digit][k][N].
struct RelinShare {
  uint32_t round = 0, N = 0, n_digits = 0;
  std::vector<u64> primes;
  std::vector<u64> data; // NTT form, canonical
};
// the derived common seeds [n_digits][32] of the public relinearization-key seeds [n_digits][32] (csprng.h relin_round_seed)
inline std::vector<uint8_t> relin_round_seeds(const std::vector<uint8_t> &relin_seeds) {
  std::vector<uint8_t> out(relin_seeds.size());
  for (size_t J = 0; J + 1 <= relin_seeds.size() / 32; J++) relin_round_seed(relin_seeds.data() + 32 * J, out.data() + 32 * J);
  return out;
}
// are the rows [..][k][N] canonical residues of their primes (row r under prime r % k)?  What the kernels' lazy-reduction
// bounds assume of every key word, asked of words that did not come through a file (serialization.h check_residues)
inline bool residues_canonical(const std::vector<u64> &words, const HostContext &h) {
  const size_t N = h.N, rows = words.size() / N;
  for (size_t r = 0; r < rows; r++) {
    const u64 q = h.primes[r % h.k], *w = words.data() + r * N;
    for (size_t j = 0; j < N; j++)
      if (w[j] >= q) return false;
  }
  return true;
}
inline void relin_round_checks(const HostContext &cx, const SecretKey &sk, uint32_t n_digits) {
  if (n_digits == 0 || n_digits > cx.k - 1) throw std::invalid_argument("invalid key digit count");
  if (sk.s_ntt.size() != (size_t)cx.k * cx.N) throw std::invalid_argument("secret key not present");
}
// round 1: h0[J][i] = -(a_J[i] u_J[i]) + NTT_i(e0_J) + [i == J] (P mod q_J) s[i],  h1[J][i] = a_J[i] s[i] + NTT_i(e1_J), with
// a_J[i] = seeded_limb(seeds[J], i) and (u_J, e0_J, e1_J) = sampled_small(r1keys[J], 0 / 1 / 2) -> [n_digits][2][k][N]
inline std::vector<u64> relin_round1_host(const HostContext &cx, const SecretKey &sk, uint32_t n_digits, const uint8_t *seeds,
                                          const std::array<uint8_t, 32> *r1keys) {
  relin_round_checks(cx, sk, n_digits);
  const uint32_t N = cx.N, k = cx.k;
  const size_t poly = (size_t)k * N;
  const u64 P = cx.primes[k - 1];
  std::vector<u64> out((size_t)n_digits * 2 * poly), a(N), un(N), en(N);
  std::vector<int8_t> p(N);
  for (uint32_t J = 0; J < n_digits; J++) {
    std::vector<int8_t> small = sampled_small3(r1keys[J], N);
    for (uint32_t i = 0; i < k; i++) {
      const u64 q = cx.primes[i], *s = sk.s_ntt.data() + (size_t)i * N;
      seeded_limb(seeds + (size_t)32 * J, i, q, N, (uint64_t *)a.data());
      u64 *h0 = out.data() + (size_t)2 * J * poly + (size_t)i * N, *h1 = h0 + poly;
      std::copy_n(small.begin(), N, p.begin());
      cx.small_to_ntt(p, i, un.data());
      std::copy_n(small.begin() + N, N, p.begin());
      cx.small_to_ntt(p, i, en.data());
      for (uint32_t j = 0; j < N; j++) h0[j] = evah::addmod(evah::negmod(cx.mulm(a[j], un[j], i), q), en[j], q);
      if (i == J) {
        const u64 pmod = P % q;
        for (uint32_t j = 0; j < N; j++) h0[j] = evah::addmod(h0[j], cx.mulm(s[j], pmod, i), q);
      }
      std::copy_n(small.begin() + (size_t)2 * N, N, p.begin());
      cx.small_to_ntt(p, i, en.data());
      for (uint32_t j = 0; j < N; j++) h1[j] = evah::addmod(cx.mulm(a[j], s[j], i), en[j], q);
    }
    wipe(small);
  }
  wipe(p);
  wipe_bytes(un.data(), un.size() * sizeof(u64));
  wipe_bytes(en.data(), en.size() * sizeof(u64));
  return out;
}
// round 2: g[J][i] = s[i] H0[J][i] + NTT_i(e2_J) + (u_J[i] - s[i]) H1[J][i] + NTT_i(e3_J), (H0, H1) = agg1[J], u_J =
// sampled_small(r1keys[J], 0), (e2_J, e3_J) = sampled_small(r2keys[J], 1 / 2) -> [n_digits][k][N]
inline std::vector<u64> relin_round2_host(const HostContext &cx, const SecretKey &sk, uint32_t n_digits, const u64 *agg1,
                                          const std::array<uint8_t, 32> *r1keys, const std::array<uint8_t, 32> *r2keys) {
  relin_round_checks(cx, sk, n_digits);
  const uint32_t N = cx.N, k = cx.k;
  const size_t poly = (size_t)k * N;
  std::vector<u64> out((size_t)n_digits * poly), un(N), e2(N), e3(N);
  std::vector<int8_t> u(N), e(N);
  for (uint32_t J = 0; J < n_digits; J++) {
    sampled_small(r1keys[J].data(), 0, N, u.data());
    for (uint32_t i = 0; i < k; i++) {
      const u64 q = cx.primes[i], *s = sk.s_ntt.data() + (size_t)i * N;
      const u64 *H0 = agg1 + (size_t)2 * J * poly + (size_t)i * N, *H1 = H0 + poly;
      cx.small_to_ntt(u, i, un.data());
      sampled_small(r2keys[J].data(), 1, N, e.data());
      cx.small_to_ntt(e, i, e2.data());
      sampled_small(r2keys[J].data(), 2, N, e.data());
      cx.small_to_ntt(e, i, e3.data());
      u64 *g = out.data() + (size_t)J * poly + (size_t)i * N;
      for (uint32_t j = 0; j < N; j++)
        g[j] = evah::addmod(evah::addmod(cx.mulm(s[j], H0[j], i), e2[j], q),
                            evah::addmod(cx.mulm(evah::submod(un[j], s[j], q), H1[j], i), e3[j], q), q);
    }
  }
  wipe(u);
  wipe(e);
  wipe_bytes(un.data(), un.size() * sizeof(u64));
  wipe_bytes(e2.data(), e2.size() * sizeof(u64));
  wipe_bytes(e3.data(), e3.size() * sizeof(u64));
  return out;
}

} // namespace evahost
