// client.hip — the host-side neighbours of execute() on the device:
// public-key encryption of an encoded plaintext and decryption + decoding of a result, i.e. the
// arithmetic of SEALPublic::encrypt and SEALSecret::decrypt (/root/reference/eva/seal/seal.cpp:24-102,
// 124-146: encoder.encode + encryptor.encrypt; decryptor.decrypt + encoder.decode).  Randomness stays on the host (csprng.h): the sampled small polynomials
// travel as int8 arrays (3 N bytes per encryption); everything of size N log N or l N runs here.
//   encrypt  : c = (pk0 u + e0, pk1 u + e1) at l+1 limbs, divided-and-rounded by the extra prime
//              (same rule as rescale A.5), plus the plaintext on c0
//   encrypt_symmetric : c1 = a expanded from a 32-byte seed (seeded.hip.h), c0 = pt - (a s + NTT(e)) at pt's limbs
//   decrypt  : m = c0 + c1 s (+ c2 s^2) per limb, inverse transform, exact recomposition to base-2^64
//              words (mixed-radix digits first), the words to one double in SEAL 3.6's order with
//              1/scale folded in and the sign taken against (Q+1)/2, forward special FFT
//              (CKKSEncoder::decode_internal), slot values out.  FP64 with SEAL's operation order and no
//              FMA contraction: the doubles are those of the oracle's evo_decode and of the host
//              decoder, bit for bit (tests/test_decode_parity.py)

#include "launch.hip.h"
#include "client.hip.h"
#include "seeded.hip.h"

namespace evah {

__global__ void __launch_bounds__(256)
k_small_to_residues(DevCtx cx, const int8_t *small, uint32_t n_polys, uint32_t limbs, u64 *out) {
  // out[p][i][n] = small[p][n] mod primes[i] (negative -> q - |v|)
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, p = blockIdx.z;
  (void)n_polys;
  const int v = small[(size_t)p * cx.N + n];
  const u64 q = cx.primes[cx.prime_of(i)].q;
  out[((size_t)p * limbs + i) * cx.N + n] = v < 0 ? q - (u64)(-v) : (u64)v;
}
// NTT forms [n_polys][limbs][N] of n_polys small polynomials (int8 [n_polys][N] on the device) under the chain primes
// 0 .. limbs - 1, on the calling queue: what evah_encrypt_symmetric and evah_keygen_switch (seeded.hip) make of their errors
void small_to_ntt(evah_ctx *c, const u64 *small8, uint32_t n_polys, uint32_t limbs, u64 *out) {
  EW_LAUNCH(k_small_to_residues, dim3(c->N / 256, limbs, n_polys), dim3(256), 0, c->stream, c->dev, reinterpret_cast<const int8_t *>(small8), n_polys, limbs, out);
  OpPlain::Params fp{out, out, (size_t)limbs * c->N, (size_t)limbs * c->N, limbs, 0, 0, {}};
  ntt_forward<OpPlain>(c, fp, n_polys * limbs);
}
// c[K][i] = pk[K][i] * u[i] + e_K[i]; small = NTT forms [3][up][N] of (u, e0, e1); pk [2][k][N]
__global__ void __launch_bounds__(256)
k_encrypt_zero(DevCtx cx, const u64 *pk, const u64 *small, uint32_t up, u64 *c) {
  const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = blockIdx.y, K = blockIdx.z;
  const DevPrime pm = cx.primes[i];
  const u64 u = small[(size_t)i * cx.N + n], e = small[((size_t)(1 + K) * up + i) * cx.N + n];
  const u64 p = pk[((size_t)K * cx.k + i) * cx.N + n];
  c[((size_t)K * up + i) * cx.N + n] = addmod(mulmod(p, u, pm), e, pm.q);
}
// c1 = a, c0 = m - (a s + en) for l limbs; m (NTT plaintext) [l][N], en (NTT error) [l][N], sk [k][N] by prime
__global__ void __launch_bounds__(256)
k_encrypt_symmetric(DevCtx cx, Seeds8 seed, const u64 *m, const u64 *en, const u64 *sk, uint32_t l, u64 *c0, u64 *c1) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (t >= cx.N / 4 || i >= l) return;
  const uint32_t prime = cx.prime_of(i);
  const DevPrime pm = cx.primes[prime];
  u64 a[4];
  seeded_block(seed.w[0], prime, t, pm, a);
  const size_t off = (size_t)i * cx.N + 4 * (size_t)t;
  const u64 *s = sk + (size_t)prime * cx.N + 4 * (size_t)t;
  const ulonglong2 m01 = ld2(m + off), m23 = ld2(m + off + 2), e01 = ld2(en + off), e23 = ld2(en + off + 2);
  const ulonglong2 s01 = ld2(s), s23 = ld2(s + 2);
  const u64 mv[4] = {m01.x, m01.y, m23.x, m23.y}, ev[4] = {e01.x, e01.y, e23.x, e23.y}, sv[4] = {s01.x, s01.y, s23.x, s23.y};
  u64 b[4];
#pragma unroll
  for (int r = 0; r < 4; r++) b[r] = submod(mv[r], addmod(mulmod(a[r], sv[r], pm), ev[r], pm.q), pm.q);
  st2(c1 + off, make_ulonglong2(a[0], a[1]));
  st2(c1 + off + 2, make_ulonglong2(a[2], a[3]));
  st2(c0 + off, make_ulonglong2(b[0], b[1]));
  st2(c0 + off + 2, make_ulonglong2(b[2], b[3]));
}

// m[i] = c0 + c1 s + c2 s^2 (size 2 or 3; a size-1 value is its own message)
__global__ void __launch_bounds__(256)
k_decrypt_dot(DevCtx cx, const u64 *ct, size_t ps, uint32_t size, const u64 *sk, u64 *m) {
  const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = blockIdx.y;
  const DevPrime pm = cx.primes[i];
  const size_t off = (size_t)i * cx.N + n;
  const u64 s = sk[off];
  u64 acc = ct[off], sp = s;
  for (uint32_t p = 1; p < size; p++) {
    acc = addmod(acc, mulmod(ct[p * ps + off], sp, pm), pm.q);
    sp = mulmod(sp, s, pm);
  }
  m[off] = acc;
}
// one double per decrypted coefficient (crt_to_double, client.hip.h), as the real part of the FFT's input
__global__ void __launch_bounds__(256)
k_crt_to_double(DevCtx cx, CrtTab t, uint32_t l, const u64 *coeff, double inv_scale, double2 *out) {
  const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  out[n] = make_double2(crt_to_double(cx, t, l, coeff, n, inv_scale), 0.0);
}
// forward special FFT stage (Cooley-Tukey): group g of `groups` uses roots[groups + g]
// (DWTHandler::transform_to_rev of SEAL 3.6: x = u + v r, y = u - v r; the complex product as four rounded
// multiplies, a rounded difference and a rounded sum — no FMA contraction, as in the encoder)
__global__ void __launch_bounds__(256)
k_dec_fft_stage(double2 *c, const double2 *roots, uint32_t groups, uint32_t log_gap, uint32_t half_n) {
#pragma clang fp contract(off)
  const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= half_n) return;
  const uint32_t gap = 1u << log_gap, g = idx >> log_gap, j = idx & (gap - 1);
  const uint32_t a = 2 * g * gap + j, b = a + gap;
  const double2 w = roots[groups + g], u = c[a], y = c[b];
  const double ac = y.x * w.x, bd = y.y * w.y, ad = y.x * w.y, bc = y.y * w.x;
  const double tx = ac - bd, ty = ad + bc;
  c[a] = make_double2(u.x + tx, u.y + ty);
  c[b] = make_double2(u.x - tx, u.y - ty);
}
__global__ void __launch_bounds__(256)
k_dec_gather(const double2 *c, const uint32_t *slot_map, uint32_t n_out, double *out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_out) out[i] = c[slot_map[i]].x;
}

} // namespace evah

extern "C" {

// the public key [2][k][N] / the secret key in NTT form [k][N] (client side), resident like the other keys
int evah_client_key_upload(evah_ctx *c, int kind, const uint64_t *data) {
  API_BEGIN
  use(c);
  if (kind != EVAH_KEY_PUBLIC && kind != EVAH_KEY_SECRET) throw std::invalid_argument("unknown key kind");
  KeyDev kd;
  kd.n_digits = 1;
  kd.bytes = sizeof(u64) * (size_t)(kind == EVAH_KEY_PUBLIC ? 2 : 1) * c->k * c->N;
  HIPCHK(hipMalloc(&kd.d, kd.bytes));
  h2d_now(c, kd.d, data, kd.bytes);
  KeyDev &slot = kind == EVAH_KEY_PUBLIC ? c->sh->pk : c->sh->sk;
  if (slot.d) {
    if (kind == EVAH_KEY_SECRET) (void)hipMemset(slot.d, 0, slot.bytes); // no key material in freed HBM
    (void)hipFree(slot.d);
  }
  slot = kd;
  API_END
}

// SEAL Encryptor::encrypt of an NTT-form plaintext with the caller's randomness: small = (u ternary,
// e0, e1 error polynomials) as int8 [3][N]
int evah_encrypt(evah_ctx *c, const evah_pt *pt, const int8_t *small, evah_ct **out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (!c->sh->pk.d) throw std::invalid_argument("public key not present");
  acquire(c, pt->buf);
  const uint32_t l = pt->limbs, up = l + 1;
  if (up > c->k) throw std::invalid_argument("plaintext level is not valid for encryption");
  const size_t N = c->N;
  Scratch sm8(c, (3 * N + 7) / 8), sm(c, (size_t)3 * up * N), ct(c, (size_t)2 * up * N), r(c, 2 * N);
  HIPCHK(hipMemcpyAsync(sm8.d, small, 3 * N, hipMemcpyHostToDevice, c->stream));
  EW_LAUNCH(k_small_to_residues, dim3(c->N / 256, up, 3), dim3(256), 0, c->stream, c->dev, reinterpret_cast<const int8_t *>(sm8.d), 3u, up, sm.d);
  OpPlain::Params fp{sm.d, sm.d, (size_t)up * N, (size_t)up * N, up, 0, 0, {}};
  ntt_forward<OpPlain>(c, fp, 3 * up);
  EW_LAUNCH(k_encrypt_zero, dim3(c->N / 256, up, 2), dim3(256), 0, c->stream, c->dev, c->sh->pk.d, sm.d, up, ct.d);
  HIPCHK(hipGetLastError());
  // divide and round by prime `l` (the last of the up primes), then add the plaintext to c0
  evah_ct *o = ct_new(c, 2, l, pt->scale);
  try {
    OpPlain::Params ip{ct.d + (size_t)l * N, r.d, (size_t)up * N, N, 1, l, 1, {}};
    ntt_inverse<OpPlain>(c, ip, 2);
    OpModDown::Params mp{r.d, N, ct.d, (size_t)up * N, pt->d, 0, 1, o->d, o->ps, l, l};
    ntt_forward<OpModDown>(c, mp, 2 * l);
    HIPCHK(hipStreamSynchronize(c->stream)); // `small` is pageable host memory
  } catch (...) {
    evah_ct_free(c, o);
    throw;
  }
  *out = o;
  API_END
}

// Encryptor::encrypt_symmetric of an NTT-form plaintext: e = one error polynomial as int8 [N] (the caller's
// sampler), a from seed32; c1 = a, c0 = pt - (a s + NTT(e)) at pt's limbs
int evah_encrypt_symmetric(evah_ctx *c, const evah_pt *pt, const int8_t *e, const uint8_t *seed32, evah_ct **out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (!c->sh->sk.d) throw std::invalid_argument("secret key not present");
  if (!e || !seed32) throw std::invalid_argument("error polynomial and seed are required");
  if (c->N % 256) throw std::invalid_argument("encryption needs N divisible by 256");
  const uint32_t l = pt->limbs;
  if (l < 1 || l > c->k - 1) throw std::invalid_argument("plaintext level is not valid for encryption"); // no special prime
  acquire(c, pt->buf);
  const size_t N = c->N;
  Scratch e8(c, (N + 7) / 8), en(c, (size_t)l * N);
  HIPCHK(hipMemcpyAsync(e8.d, e, N, hipMemcpyHostToDevice, c->stream));
  small_to_ntt(c, e8.d, 1, l, en.d);
  evah_ct *o = ct_new(c, 2, l, pt->scale);
  try {
    const Seeds8 s = seeds_of(&seed32, 0, 1);
    EW_LAUNCH(k_encrypt_symmetric, seeded_grid(c, l, 1), dim3(256), 0, c->stream, c->dev, s, pt->d, en.d, c->sh->sk.d, l, o->d, o->d + o->ps);
    HIPCHK(hipGetLastError());
    // the error does not stay behind in pool memory the next call reuses
    HIPCHK(hipMemsetAsync(en.d, 0, sizeof(u64) * (size_t)l * N, c->stream));
    HIPCHK(hipMemsetAsync(e8.d, 0, N, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // `e` is pageable host memory
  } catch (...) {
    evah_ct_free(c, o);
    throw;
  }
  *out = o;
  API_END
}

// SEAL Decryptor::decrypt + CKKSEncoder::decode: the first n_out slot values of the message of ct
int evah_decrypt_decode(evah_ctx *c, const evah_ct *ct, uint32_t n_out, double *out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (!c->sh->sk.d) throw std::invalid_argument("secret key not present");
  if (ct->batch != 1) throw std::invalid_argument("decrypt takes a single ciphertext");
  acquire(c, ct->buf);
  const uint32_t l = ct->limbs, N = c->N, slots = N >> 1;
  if (n_out < 1 || n_out > slots) throw std::invalid_argument("slot count out of range");
  if (l > 61) throw std::invalid_argument("too many limbs");
  check_scale(c, ct->scale, l); // decode_internal: "scale out of bounds"
  enc_tables(c);
  dec_tables(c);
  const std::vector<u64> tab = crt_tab_build(c, l); // Garner tables of this level
  Scratch m(c, (size_t)l * N), tabd(c, tab.size()), cbuf(c, 2 * (size_t)N), outd(c, n_out);
  HIPCHK(hipMemcpyAsync(tabd.d, tab.data(), sizeof(u64) * tab.size(), hipMemcpyHostToDevice, c->stream));
  EW_LAUNCH(k_decrypt_dot, dim3(N / 256, l), dim3(256), 0, c->stream, c->dev, ct->d, ct->ps, ct->size, c->sh->sk.d, m.d);
  OpPlain::Params ip{m.d, m.d, 0, 0, l, 0, 0, {}};
  ntt_inverse<OpPlain>(c, ip, l);
  const CrtTab t = crt_tab_at(tabd.d, l);
  double2 *cd = reinterpret_cast<double2 *>(cbuf.d);
  EW_LAUNCH(k_crt_to_double, dim3(N / 256), dim3(256), 0, c->stream, c->dev, t, l, m.d, 1.0 / ct->scale, cd);
  // the decrypted message and its FP image do not stay behind in pool memory the next call reuses
  HIPCHK(hipMemsetAsync(m.d, 0, sizeof(u64) * (size_t)l * N, c->stream));
  for (uint32_t groups = 1, lg = c->logN - 1; groups < N; groups <<= 1, lg--)
    hipLaunchKernelGGL(k_dec_fft_stage, dim3((slots + 255) / 256), dim3(256), 0, c->stream, cd, c->sh->dec_roots, groups, lg, slots);
  hipLaunchKernelGGL(k_dec_gather, dim3((n_out + 255) / 256), dim3(256), 0, c->stream, cd, c->sh->enc_slot_map, n_out,
                     reinterpret_cast<double *>(outd.d));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, outd.d, sizeof(double) * n_out, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemsetAsync(cbuf.d, 0, sizeof(double2) * (size_t)N, c->stream));
  HIPCHK(hipMemsetAsync(outd.d, 0, sizeof(double) * n_out, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  API_END
}

} // extern "C"
