// seeded.hip — ciphertexts whose second polynomial travels as a 32-byte seed (SEAL's Encryptor::encrypt_symmetric
// followed by a seeded save): uploads of c0 + seed with c1 expanded on the queue (the expansion rule:
// seeded.hip.h), slot refills of captured graphs, and the download of c0 alone.  The fused symmetric encryption
// (evah_encrypt_symmetric and its _many forms) lives in client.hip beside the public-key one.  Evaluation keys travel the same way:
// evah_key_upload_seeded takes c0 and one seed per digit and expands every c1 row — and the split copy — in one launch.
// evah_keygen_switch makes the whole key here: c0 as well, from the resident secret key and N int8 error
// draws per digit.  evah_keygen_set makes a whole set of them, and evah_keygen_public the public key, from
// 32-byte randomness keys the device expands itself — one k_keygen_set launch for the set —, and evah_key_download_c0
// hands c0 of such a key to the host when it is first needed there.  evah_keygen_rekey makes the key
// that takes ciphertexts to ANOTHER key pair, from that pair's public key: one k_keygen_rekey launch.
// evah_keygen_relin_round1 / _round2 make a party's two shares of a committee's relinearization key:
// one k_relin_round1 / k_relin_round2 launch each.
// What the generators share is written once: on the device the key equation (key_row, called by k_keygen_switch and
// k_keygen_set), the seed fetch and the four-coefficient accessors (seeded.hip.h); on the host the refusals
// (keygen_checks, keygen_ready, switch_kind_checks), the seeds of a launch (SeedArgs), the key's allocations (KeyAlloc,
// internal.hip.h), the c0 copies (c0_download) and the frame that drains the queue on success and on failure (drained).

#include "launch.hip.h"
#include "seeded.hip.h"

namespace evah {

// c1 of instance z: dst + z * inst_stride holds limbs [limbs][N]; one thread per ChaCha block (4 coefficients);
// grid = (ceil(N / 4 / 256), limbs, instances of this launch)
__global__ void __launch_bounds__(256)
k_expand_seeded(DevCtx cx, Seeds8 seeds, uint32_t limbs, u64 *dst, size_t inst_stride) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, z = blockIdx.z;
  if (t >= cx.N / 4 || i >= limbs) return;
  const uint32_t prime = cx.prime_of(i);
  const DevPrime pm = cx.primes[prime];
  u64 a[4];
  seeded_block(seeds.w[z], prime, t, pm, a);
  st4(dst + z * inst_stride + (size_t)i * cx.N + 4 * (size_t)t, a);
}

// c1 of `batch` instances of ct from their seeds: instance b's c1 starts at ct->d + b * 2 * ps + ps
static void expand_c1(evah_ctx *c, evah_ct *ct, const uint8_t *const *seeds) {
  for (uint32_t b0 = 0; b0 < ct->batch; b0 += SEEDS_PER_LAUNCH) {
    const uint32_t n = std::min(SEEDS_PER_LAUNCH, ct->batch - b0);
    const Seeds8 s = seeds_of(seeds, b0, n);
    EW_LAUNCH(k_expand_seeded, seeded_grid(c, ct->limbs, n), dim3(256), 0, c->stream, c->dev, s, ct->limbs,
              ct->d + ((size_t)b0 * 2 + 1) * ct->ps, 2 * ct->ps);
  }
  HIPCHK(hipGetLastError());
}

// The c1 half of a seed-compressed evaluation key in the device layout d = [digit][2][rows][N]: row r of
// digit J is seeded_block(seed_J, prime of r, .) — every chain prime of a whole key; the data limbs s, s + G, ... and then
// the special prime on a limb shard.  When the key has a split copy (KeyDev::d_split) the same launch writes both of its
// halves: split(c1) from the registers and split(c0) from the words the upload's copies left in d[J][0][r], so no pass
// reads the whole key again.  One thread per ChaCha block (4 coefficients); grid = (ceil(N / 4 / 256), rows, digits).
// Seeds: launch arguments for up to 8 digits, else seed_buf ([digits][8] words, uploaded on the same queue).
__global__ void __launch_bounds__(256)
k_key_expand(DevCtx cx, Seeds8 seeds, const uint32_t *__restrict__ seed_buf, uint32_t rows, u64 *__restrict__ d, u64 *__restrict__ d_split) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y, J = blockIdx.z;
  if (t >= cx.N / 4 || r >= rows) return;
  const uint32_t prime = cx.pstep > 1 && r + 1 == rows ? cx.k - 1 : cx.prime_of(r);
  const DevPrime pm = cx.primes[prime];
  uint32_t key[8];
  seed_words(seeds, seed_buf, J, key);
  u64 a[4];
  seeded_block(key, prime, t, pm, a);
  const size_t at0 = ((size_t)2 * J * rows + r) * cx.N + 4 * (size_t)t, at1 = at0 + (size_t)rows * cx.N;
  st4(d + at1, a);
  if (d_split) {
    st4_split(d_split + at1, a);
    u64 b[4];
    ld4(d + at0, b);
    st4_split(d_split + at0, b);
  }
}

// what s' of a key-switching key is: s^2 (relinearization), s through the Galois element's permutation table, or no s'
// row at all (the public key)
enum : uint32_t { KS_SPRIME_SQUARE = 0, KS_SPRIME_PERM = 1, KS_SPRIME_NONE = 2 };

// The key equation, one thread's four coefficients of digit J, chain prime i of a key in the device layout
// d = [digit][2][k][N]: a = seeded_block(key, i, t), c0 = -(a s + NTT(e)) and, on the row i == J (uniform over the block)
// of a key that has an s', + (P mod q_J) s'.  s' is never stored: s * s, or s read through perm (the table rotations use:
// s'[n] = s[perm[n]]).  e: row i of the digit's NTT-form error; sk [k][N].  Both polynomials and, when the key has one,
// the split copy leave from the same registers, 16 bytes per access.
__device__ __forceinline__ void key_row(const DevCtx &cx, const uint32_t key[8], uint32_t i, uint32_t J, uint32_t t, const u64 *e, const u64 *sk,
                                        uint32_t sprime, const uint32_t *perm, u64 *d, u64 *d_split) {
  const DevPrime pm = cx.primes[i];
  u64 a[4], b[4], sv[4], ev[4];
  seeded_block(key, i, t, pm, a);
  const size_t n0 = 4 * (size_t)t;
  const u64 *s = sk + (size_t)i * cx.N;
  ld4(s + n0, sv);
  ld4(e + n0, ev);
#pragma unroll
  for (int r = 0; r < 4; r++) b[r] = negmod(addmod(mulmod(a[r], sv[r], pm), ev[r], pm.q), pm.q);
  if (i == J && sprime != KS_SPRIME_NONE) {
    const u64 pmod = cx.modq[(size_t)(cx.k - 1) * cx.k + J].x; // P mod q_J
    u64 sp[4];
    if (sprime == KS_SPRIME_PERM) {
      const uint4 pi = *reinterpret_cast<const uint4 *>(perm + n0);
      sp[0] = s[pi.x]; sp[1] = s[pi.y]; sp[2] = s[pi.z]; sp[3] = s[pi.w];
    } else {
#pragma unroll
      for (int r = 0; r < 4; r++) sp[r] = mulmod(sv[r], sv[r], pm);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) b[r] = addmod(b[r], mulmod(sp[r], pmod, pm), pm.q);
  }
  const size_t at0 = ((size_t)2 * J * cx.k + i) * cx.N + n0, at1 = at0 + (size_t)cx.k * cx.N;
  st4(d + at0, b);
  st4(d + at1, a);
  if (d_split) {
    st4_split(d_split + at0, b);
    st4_split(d_split + at1, a);
  }
}

// A whole key-switching key from the secret key and seeds: key_row for digit J = blockIdx.z and chain
// prime i = blockIdx.y, with s' = s * s for the relinearization key (perm == nullptr) and s through perm otherwise.
// en = NTT(e) [digit][k][N].  One thread per ChaCha block (4 coefficients); grid = (ceil(N / 4 / 256), k, digits).
// Seeds as in k_key_expand.
__global__ void __launch_bounds__(256)
k_keygen_switch(DevCtx cx, Seeds8 seeds, const uint32_t *__restrict__ seed_buf, const u64 *__restrict__ en, const u64 *__restrict__ sk,
                const uint32_t *__restrict__ perm, u64 *__restrict__ d, u64 *__restrict__ d_split) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, J = blockIdx.z;
  if (t >= cx.N / 4 || i >= cx.k) return;
  uint32_t key[8];
  seed_words(seeds, seed_buf, J, key);
  key_row(cx, key, i, J, t, en + ((size_t)J * cx.k + i) * cx.N, sk, perm ? KS_SPRIME_PERM : KS_SPRIME_SQUARE, perm, d, d_split);
}

// One key of a set, read wave-uniformly by k_keygen_set: where its words go and what s' is
struct KeySetEntry {
  u64 *d, *d_split;     // [digit][2][k][N] each; d_split null: no split copy
  const uint32_t *perm; // KS_SPRIME_PERM: the Galois element's permutation table
  uint32_t sprime, pad; // KS_SPRIME_*
};

// k_keygen_switch for every key of a set in one launch: blockIdx.z = key * n_digits + J; the key's
// {d, d_split, perm, sprime} come from tab[key], digit z's seed from seed_buf [z][8] and its NTT-form error from en
// [z][k][N] (z counts within the launch); key_row does the rest.  A one-entry table with KS_SPRIME_NONE and one digit is
// the public key (-(a s + NTT(e)), a) in its [2][k][N] layout.  grid = (ceil(N / 4 / 256), k, keys * n_digits)
__global__ void __launch_bounds__(256)
k_keygen_set(DevCtx cx, const uint32_t *__restrict__ seed_buf, const u64 *__restrict__ en, const u64 *__restrict__ sk,
             const KeySetEntry *__restrict__ tab, uint32_t n_digits) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, z = blockIdx.z;
  if (t >= cx.N / 4 || i >= cx.k) return;
  const KeySetEntry ke = tab[z / n_digits];
  uint32_t key[8];
#pragma unroll
  for (int w = 0; w < 8; w++) key[w] = seed_buf[8 * (size_t)z + w];
  key_row(cx, key, i, z % n_digits, t, en + ((size_t)z * cx.k + i) * cx.N, sk, ke.sprime, ke.perm, ke.d, ke.d_split);
}

// the first polynomial of every digit of a key d [digit][2][k][N] -> out [digit][k][N] (host), enqueued: one linear copy
// per digit (evah_ct_download on 2-D copies and pageable memory)
static void c0_download(evah_ctx *c, const u64 *d, uint32_t n_digits, uint64_t *out) {
  const size_t poly = (size_t)c->k * c->N;
  for (uint32_t J = 0; J < n_digits; J++)
    HIPCHK(hipMemcpyAsync(out + (size_t)J * poly, d + (size_t)J * 2 * poly, sizeof(u64) * poly, hipMemcpyDeviceToHost, c->stream));
}

// The keys [first, first + n) of a set — or the public key (n = 1, one digit) — into their allocations tab[.].d: the
// launch list of DESIGN.md 1.8.  ekeys / seeds [n][n_digits][32] (host); out (host, or null): entry j's first polynomial
// of every digit, [n_digits][k][N] each, from d[J][0].  Enqueues only: the caller drains the queue.
static void keygen_chunk(evah_ctx *c, const KeySetEntry *tab, uint32_t n, uint32_t n_digits, const uint8_t *ekeys, const uint8_t *seeds,
                         uint64_t *out) {
  const size_t Z = (size_t)n * n_digits, poly = (size_t)c->k * c->N, tab_words = (sizeof(KeySetEntry) * n + 7) / 8;
  Scratch ek(c, 4 * Z), sd(c, 4 * Z), tb(c, tab_words), en(c, Z * poly);
  // the error keys, the sampled residues and their NTT forms do not stay behind in pool memory the next call reuses
  Wipe w_ek{c, ek.d, 32 * Z}, w_en{c, en.d, sizeof(u64) * Z * poly};
  HIPCHK(hipMemcpyAsync(sd.d, seeds, 32 * Z, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(tb.d, tab, sizeof(KeySetEntry) * n, hipMemcpyHostToDevice, c->stream));
  sample_to_ntt(c, (uint32_t)Z, ekeys, ek.d, 1, 1, c->k, en.d);
  EW_LAUNCH(k_keygen_set, seeded_grid(c, c->k, (uint32_t)Z), dim3(256), 0, c->stream, c->dev, reinterpret_cast<const uint32_t *>(sd.d), en.d,
            c->sh->sk.d, reinterpret_cast<const KeySetEntry *>(tb.d), n_digits);
  HIPCHK(hipGetLastError());
  if (out)
    for (uint32_t j = 0; j < n; j++) c0_download(c, tab[j].d, n_digits, out + (size_t)j * n_digits * poly);
  w_ek.now();
  w_en.now();
}

// The re-key key to another key pair from that pair's public key: digit J, prime row i is the public-key
// zero encryption k_encrypt_zero forms — pk_K u_J + e_K,J — with [i == J] (P mod q_J) s_i added to K = 0, both polynomials
// from one read of u.  small: the NTT forms [digit][3][k][N] of (u, e0, e1); pk [2][k][N]; sk [k][N]; d [digit][2][k][N].
// One thread per two coefficients, 16-byte accesses; the i == J branch is uniform over the block.
// grid = (ceil(N / 2 / 256), k, n_digits)
__global__ void __launch_bounds__(256)
k_keygen_rekey(DevCtx cx, const u64 *__restrict__ pk, const u64 *__restrict__ small, const u64 *__restrict__ sk, u64 *__restrict__ d) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, J = blockIdx.z;
  if (2 * t >= cx.N || i >= cx.k) return;
  const DevPrime pm = cx.primes[i];
  const size_t poly = (size_t)cx.k * cx.N, row = (size_t)i * cx.N + 2 * (size_t)t;
  const u64 *sm = small + (size_t)J * 3 * poly + row;
  const ulonglong2 u = ld2(sm), e0 = ld2(sm + poly), e1 = ld2(sm + 2 * poly), p0 = ld2(pk + row), p1 = ld2(pk + poly + row);
  ulonglong2 b0, b1;
  b0.x = addmod(mulmod(p0.x, u.x, pm), e0.x, pm.q);
  b0.y = addmod(mulmod(p0.y, u.y, pm), e0.y, pm.q);
  b1.x = addmod(mulmod(p1.x, u.x, pm), e1.x, pm.q);
  b1.y = addmod(mulmod(p1.y, u.y, pm), e1.y, pm.q);
  if (i == J) {
    const u64 pmod = cx.modq[(size_t)(cx.k - 1) * cx.k + J].x; // P mod q_J
    const ulonglong2 s = ld2(sk + row);
    b0.x = addmod(b0.x, mulmod(s.x, pmod, pm), pm.q);
    b0.y = addmod(b0.y, mulmod(s.y, pmod, pm), pm.q);
  }
  u64 *at = d + (size_t)2 * J * poly + row;
  st2(at, b0);
  st2(at + poly, b1);
}

// Round 1 of the collective relinearization key: this party's share of digit J, prime row i,
//   h0 = -(a u_J) + NTT(e0_J) + [i == J] (P mod q_J) s,   h1 = a s + NTT(e1_J),
// with a = seeded_block(seed'_J, i, .) in registers only — the common row every party expands, never stored.  small: the
// NTT forms [digit][3][k][N] of (u, e0, e1); sk [k][N], read once for both polynomials; out [digit][2][k][N], both halves
// from the same registers.  One thread per ChaCha block (4 coefficients), 16-byte accesses; the i == J branch is uniform
// over the block.  grid = (ceil(N / 4 / 256), k, digits).  Seeds as in k_key_expand.
__global__ void __launch_bounds__(256)
k_relin_round1(DevCtx cx, Seeds8 seeds, const uint32_t *__restrict__ seed_buf, const u64 *__restrict__ small, const u64 *__restrict__ sk,
               u64 *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, J = blockIdx.z;
  if (t >= cx.N / 4 || i >= cx.k) return;
  const DevPrime pm = cx.primes[i];
  uint32_t key[8];
  seed_words(seeds, seed_buf, J, key);
  u64 a[4], h0[4], h1[4], uv[4], e0[4], e1[4], sv[4];
  seeded_block(key, i, t, pm, a);
  const size_t poly = (size_t)cx.k * cx.N, row = (size_t)i * cx.N + 4 * (size_t)t;
  const u64 *sm = small + (size_t)J * 3 * poly + row;
  ld4(sm, uv);
  ld4(sm + poly, e0);
  ld4(sm + 2 * poly, e1);
  ld4(sk + row, sv);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    h0[r] = addmod(negmod(mulmod(a[r], uv[r], pm), pm.q), e0[r], pm.q);
    h1[r] = addmod(mulmod(a[r], sv[r], pm), e1[r], pm.q);
  }
  if (i == J) {
    const u64 pmod = cx.modq[(size_t)(cx.k - 1) * cx.k + J].x; // P mod q_J
#pragma unroll
    for (int r = 0; r < 4; r++) h0[r] = addmod(h0[r], mulmod(sv[r], pmod, pm), pm.q);
  }
  u64 *at = out + (size_t)2 * J * poly + row;
  st4(at, h0);
  st4(at + poly, h1);
}

// Round 2: g = s H0 + NTT(e2_J) + (u_J - s) H1 + NTT(e3_J) for digit J, prime row i.  agg [digit][2][k][N]
// (H0, H1: the sums of the round-1 shares); un [digit][k][N]: NTT(u_J) of this party's round-1 keys; en [digit][2][k][N]:
// NTT(e2_J), NTT(e3_J); sk [k][N]; out [digit][k][N].  One thread per two coefficients, 16-byte accesses, no branch.
// grid = (ceil(N / 2 / 256), k, digits)
__global__ void __launch_bounds__(256)
k_relin_round2(DevCtx cx, const u64 *__restrict__ agg, const u64 *__restrict__ un, const u64 *__restrict__ en, const u64 *__restrict__ sk,
               u64 *__restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, J = blockIdx.z;
  if (2 * t >= cx.N || i >= cx.k) return;
  const DevPrime pm = cx.primes[i];
  const size_t poly = (size_t)cx.k * cx.N, row = (size_t)i * cx.N + 2 * (size_t)t;
  const u64 *ag = agg + (size_t)2 * J * poly + row, *e = en + (size_t)2 * J * poly + row;
  const ulonglong2 H0 = ld2(ag), H1 = ld2(ag + poly), u = ld2(un + (size_t)J * poly + row), e2 = ld2(e), e3 = ld2(e + poly), s = ld2(sk + row);
  ulonglong2 g;
  g.x = addmod(addmod(mulmod(s.x, H0.x, pm), e2.x, pm.q), addmod(mulmod(submod(u.x, s.x, pm.q), H1.x, pm), e3.x, pm.q), pm.q);
  g.y = addmod(addmod(mulmod(s.y, H0.y, pm), e2.y, pm.q), addmod(mulmod(submod(u.y, s.y, pm.q), H1.y, pm), e3.y, pm.q), pm.q);
  st2(out + (size_t)J * poly + row, g);
}

// the refusals every generator shares: keygen_checks before it looks at its arguments, keygen_ready after
static void keygen_checks(evah_ctx *c) {
  if (c->dev.pstep > 1) throw std::invalid_argument("a limb shard holds no whole secret key");
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
}
static void keygen_ready(evah_ctx *c) {
  if (c->N % 256) throw std::invalid_argument("key generation needs N divisible by 256");
  if (!c->sh->sk.d) throw std::invalid_argument("secret key not present");
}
// the kinds of key that travel seed-compressed or are generated from seeds: relinearization and Galois; rekey_msg says
// where a re-key key goes instead
static void switch_kind_checks(evah_ctx *c, int kind, uint32_t galois_elt, const char *rekey_msg) {
  if (kind == EVAH_KEY_REKEY) throw std::invalid_argument(rekey_msg);
  if (kind != EVAH_KEY_RELIN && kind != EVAH_KEY_GALOIS) throw std::invalid_argument("unknown key kind");
  if (kind == EVAH_KEY_GALOIS && (!(galois_elt & 1) || galois_elt >= 2 * c->N)) throw std::invalid_argument("Galois element is not valid");
}
static const char *const REKEY_GENERATED = "a re-key key is generated by evah_keygen_rekey";

// body(), then the drain of the queue — also when body throws, before anything the caller holds (key allocations,
// scratch, pageable arguments) is let go
template <class F> static void drained(evah_ctx *c, F &&body) {
  try {
    body();
    HIPCHK(hipStreamSynchronize(c->stream));
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    throw;
  }
}

} // namespace evah

extern "C" {

// A relinearization or Galois key from c0 [n_digits][k][N] and one 32-byte seed per digit: what
// evah_key_upload installs for the materialised key, with half the words crossing PCIe
int evah_key_upload_seeded(evah_ctx *c, int kind, uint32_t galois_elt, uint32_t n_digits, const uint64_t *c0, const uint8_t *seeds) {
  API_BEGIN
  use(c);
  const KeyDev shape = key_shape(c, n_digits);
  switch_kind_checks(c, kind, galois_elt, "a re-key key is not seed-compressible: upload it whole (evah_key_upload)");
  if (!c0) throw std::invalid_argument("key pointer is null");
  if (!seeds) throw std::invalid_argument("seed pointer is null");
  KeyAlloc key(c, shape);
  const KeyDev &kd = key.kd;
  std::optional<SeedArgs> sa; // its device buffer (more than 8 digits) returns to the pool after the drain
  drained(c, [&] { // complete before any queue reads the rows (h2d_now)
    const size_t poly = (size_t)c->k * c->N;
    hipError_t e = hipSuccess;
    if (c->dev.pstep <= 1) // a whole key: c0 of digit J into d[J][0], one copy per digit
      for (uint32_t J = 0; J < n_digits && e == hipSuccess; J++)
        e = hipMemcpyAsync(kd.d + (size_t)J * 2 * poly, (const u64 *)c0 + (size_t)J * poly, sizeof(u64) * poly, hipMemcpyHostToDevice, c->stream);
    else
      e = key_rows_h2d(c, kd, (const u64 *)c0, n_digits, 0, 2);
    HIPCHK(e);
    sa.emplace(c, seeds, n_digits);
    EW_LAUNCH(k_key_expand, seeded_grid(c, kd.rows, n_digits), dim3(256), 0, c->stream, c->dev, sa->s8, sa->buf, kd.rows, kd.d, kd.d_split);
    HIPCHK(hipGetLastError());
  });
  key_install(c, kind, galois_elt, key.release());
  c->sh->key_up[0]++;
  c->sh->key_up[1] += shape.bytes / 2 + (size_t)32 * n_digits; // c0 of the rows kept + the seeds
  API_END
}

// A relinearization or Galois key generated on the device: the caller supplies what is random — one int8
// error polynomial and one 32-byte seed per digit — and the context's secret key does the rest; the key is installed like
// an uploaded one and / or its c0 handed back, word for word the host generator's compressed key for the same draws
int evah_keygen_switch(evah_ctx *c, int kind, uint32_t galois_elt, uint32_t n_digits, const int8_t *errors, const uint8_t *seeds,
                       int install, uint64_t *c0_out) {
  API_BEGIN
  use(c);
  keygen_checks(c);
  const KeyDev shape = key_shape(c, n_digits);
  switch_kind_checks(c, kind, galois_elt, REKEY_GENERATED);
  if (!errors) throw std::invalid_argument("error pointer is null");
  if (!seeds) throw std::invalid_argument("seed pointer is null");
  if (!install && !c0_out) throw std::invalid_argument("the key is neither installed nor returned");
  keygen_ready(c);
  const uint32_t *perm = kind == EVAH_KEY_GALOIS ? perm_table(c, galois_elt) : nullptr;
  const size_t poly = (size_t)c->k * c->N, e_bytes = (size_t)n_digits * c->N;
  KeyAlloc key(c, shape);
  Scratch e8(c, (e_bytes + 7) / 8), en(c, (size_t)n_digits * poly);
  std::optional<SeedArgs> sa; // its device buffer (more than 8 digits) returns to the pool after the drain
  drained(c, [&] { // `errors` and c0_out are pageable; complete before any queue reads the key
    // the errors do not stay behind in pool memory the next call reuses
    Wipe w_en{c, en.d, sizeof(u64) * (size_t)n_digits * poly}, w_e8{c, e8.d, e_bytes};
    HIPCHK(hipMemcpyAsync(e8.d, errors, e_bytes, hipMemcpyHostToDevice, c->stream));
    small_to_ntt(c, e8.d, n_digits, c->k, en.d);
    sa.emplace(c, seeds, n_digits);
    EW_LAUNCH(k_keygen_switch, seeded_grid(c, c->k, n_digits), dim3(256), 0, c->stream, c->dev, sa->s8, sa->buf, en.d, c->sh->sk.d, perm, key.kd.d,
              key.kd.d_split);
    HIPCHK(hipGetLastError());
    if (c0_out) c0_download(c, key.kd.d, n_digits, c0_out);
    w_en.now();
    w_e8.now();
  });
  c->sh->xfer[4] += e_bytes + (size_t)32 * n_digits;
  if (c0_out) c->sh->xfer[5] += sizeof(u64) * (size_t)n_digits * poly;
  if (install) key_install(c, kind, galois_elt, key.release());
  API_END
}

// A whole set of relinearization / Galois keys generated on the device from 32-byte randomness keys: key
// kappa, digit J is evah_keygen_switch with errors[J] = sampled_small(ekeys[kappa][J], 1), word for word, in a number of
// launches that does not depend on the number of keys.  All or nothing: a failure installs no key of the set.
int evah_keygen_set(evah_ctx *c, uint32_t n_keys, const int *kinds, const uint32_t *elts, uint32_t n_digits, const uint8_t *ekeys,
                    const uint8_t *seeds, int install, uint64_t *c0_out) {
  API_BEGIN
  use(c);
  keygen_checks(c);
  const KeyDev shape = key_shape(c, n_digits);
  if (n_keys == 0) throw std::invalid_argument("a key set needs at least one key");
  if (!kinds || !elts) throw std::invalid_argument("key list pointer is null");
  if ((uint64_t)n_keys * n_digits > 65535) throw std::invalid_argument("a key set holds at most 65535 digits");
  for (uint32_t j = 0; j < n_keys; j++) {
    switch_kind_checks(c, kinds[j], elts[j], REKEY_GENERATED);
    for (uint32_t i = 0; i < j; i++)
      if (kinds[i] == kinds[j] && (kinds[j] == EVAH_KEY_RELIN || elts[i] == elts[j]))
        throw std::invalid_argument("key " + std::to_string(j) + " repeats key " + std::to_string(i));
  }
  if (!ekeys) throw std::invalid_argument("error pointer is null");
  if (!seeds) throw std::invalid_argument("seed pointer is null");
  if (!install && !c0_out) throw std::invalid_argument("the key is neither installed nor returned");
  keygen_ready(c);
  const size_t key_words = (size_t)n_digits * c->k * c->N;
  std::vector<KeyAlloc> keys; // freed behind the drain unless every key of the set was made
  std::vector<KeySetEntry> tab(n_keys, KeySetEntry{nullptr, nullptr, nullptr, KS_SPRIME_SQUARE, 0});
  keys.reserve(n_keys);
  drained(c, [&] { // `ekeys`, `seeds` and c0_out are pageable; complete before any queue reads a key
    for (uint32_t j = 0; j < n_keys; j++) { // the permutation tables before the first launch (first use: a copy of its own)
      if (kinds[j] != EVAH_KEY_GALOIS) continue;
      tab[j].perm = perm_table(c, elts[j]);
      tab[j].sprime = KS_SPRIME_PERM;
    }
    for (KeySetEntry &ke : tab) {
      keys.emplace_back(c, shape);
      ke.d = keys.back().kd.d;
      ke.d_split = keys.back().kd.d_split;
    }
    // whole keys per launch list: as many as Tunables::keygen_set_words of NTT-form errors hold, at least one
    const uint32_t per_chunk = (uint32_t)std::min<size_t>(n_keys, std::max<size_t>(1, c->tun.keygen_set_words / key_words));
    for (uint32_t j0 = 0; j0 < n_keys; j0 += per_chunk) {
      const uint32_t n = std::min(per_chunk, n_keys - j0);
      const size_t at = (size_t)32 * j0 * n_digits;
      keygen_chunk(c, tab.data() + j0, n, n_digits, ekeys + at, seeds + at, c0_out ? c0_out + (size_t)j0 * key_words : nullptr);
    }
  });
  c->sh->xfer[4] += (size_t)64 * n_keys * n_digits;
  if (c0_out) c->sh->xfer[5] += sizeof(u64) * n_keys * key_words;
  if (install)
    for (uint32_t j = 0; j < n_keys; j++) key_install(c, kinds[j], elts[j], keys[j].release()); // cannot refuse: checked above
  API_END
}

// The public key (-(a s + NTT(e)), a) generated on the device: a_i = the expansion of seed32 under chain
// prime i, e = sampled_small(ekey32, 1) — k_keygen_set with a one-entry table and no s' row, whose one digit is exactly
// the [2][k][N] layout of the public key
int evah_keygen_public(evah_ctx *c, const uint8_t *ekey32, const uint8_t *seed32, int install, uint64_t *pk_out) {
  API_BEGIN
  use(c);
  keygen_checks(c);
  if (!ekey32) throw std::invalid_argument("error pointer is null");
  if (!seed32) throw std::invalid_argument("seed pointer is null");
  if (!install && !pk_out) throw std::invalid_argument("the key is neither installed nor returned");
  keygen_ready(c);
  KeyDev shape;
  shape.n_digits = 1;
  shape.bytes = sizeof(u64) * (size_t)2 * c->k * c->N;
  KeyAlloc key(c, shape, false); // encryption reads no split copy
  const KeyDev &kd = key.kd;
  drained(c, [&] { // the arguments are pageable; complete before any queue reads the key
    const KeySetEntry ke{kd.d, nullptr, nullptr, KS_SPRIME_NONE, 0};
    keygen_chunk(c, &ke, 1, 1, ekey32, seed32, nullptr);
    if (pk_out) HIPCHK(hipMemcpyAsync(pk_out, kd.d, kd.bytes, hipMemcpyDeviceToHost, c->stream));
  });
  c->sh->xfer[4] += 64;
  if (pk_out) c->sh->xfer[5] += kd.bytes;
  if (install) {
    if (c->sh->pk.d) (void)hipFree(c->sh->pk.d);
    c->sh->pk = key.release();
  }
  API_END
}

// The re-key key from this context's key pair to the pair whose public key is pk_target.  Launch plan:
// pk_target and the randomness keys up on the queue (into scratch: the context's own public key stays), the NTT forms of
// (u, e0, e1) of every digit (sample_to_ntt: k_sample_small + the two forward passes), ONE k_keygen_rekey, the key back.
int evah_keygen_rekey(evah_ctx *c, const uint64_t *pk_target, uint32_t n_digits, const uint8_t *rkeys, uint64_t *key_out) {
  API_BEGIN
  use(c);
  keygen_checks(c);
  const KeyDev shape = key_shape(c, n_digits);
  if (!pk_target) throw std::invalid_argument("key pointer is null");
  if (!rkeys) throw std::invalid_argument("randomness key pointer is null");
  if (!key_out) throw std::invalid_argument("output pointer is null");
  keygen_ready(c);
  const size_t poly = (size_t)c->k * c->N;
  Scratch pk(c, 2 * poly), rk(c, (size_t)4 * n_digits), sm(c, (size_t)n_digits * 3 * poly), key(c, (size_t)n_digits * 2 * poly);
  drained(c, [&] { // the arguments are pageable; the scratch returns to the pool drained
    // the randomness keys, the sampled residues and their NTT forms do not stay behind in pool memory the next call reuses
    Wipe w_rk{c, rk.d, (size_t)32 * n_digits}, w_sm{c, sm.d, sizeof(u64) * n_digits * 3 * poly};
    HIPCHK(hipMemcpyAsync(pk.d, pk_target, sizeof(u64) * 2 * poly, hipMemcpyHostToDevice, c->stream));
    sample_to_ntt(c, n_digits, rkeys, rk.d, 3, 0, c->k, sm.d);
    EW_LAUNCH(k_keygen_rekey, dim3((c->N / 2 + 255) / 256, c->k, n_digits), dim3(256), 0, c->stream, c->dev, pk.d, sm.d, c->sh->sk.d, key.d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(key_out, key.d, shape.bytes, hipMemcpyDeviceToHost, c->stream));
    w_rk.now();
    w_sm.now();
  });
  c->sh->xfer[4] += sizeof(u64) * 2 * poly + (size_t)32 * n_digits;
  c->sh->xfer[5] += shape.bytes;
  API_END
}

// Round 1 of the collective relinearization-key generation: this party's public share [n_digits][2][k][N]
// from the resident secret key, the derived common seeds (relin_round_seed) and one ephemeral 32-byte key per digit.
// Launch plan: the randomness keys (and, above SEEDS_PER_LAUNCH digits, the seeds) up, the NTT forms of (u, e0, e1) of
// every digit (sample_to_ntt), ONE k_relin_round1, the share back, the wipes, one drain.
int evah_keygen_relin_round1(evah_ctx *c, uint32_t n_digits, const uint8_t *seeds, const uint8_t *r1keys, uint64_t *share_out) {
  API_BEGIN
  use(c);
  keygen_checks(c);
  const KeyDev shape = key_shape(c, n_digits);
  if (!seeds) throw std::invalid_argument("seed pointer is null");
  if (!r1keys) throw std::invalid_argument("randomness key pointer is null");
  if (!share_out) throw std::invalid_argument("output pointer is null");
  keygen_ready(c);
  const size_t poly = (size_t)c->k * c->N;
  Scratch rk(c, (size_t)4 * n_digits), sm(c, (size_t)n_digits * 3 * poly), share(c, (size_t)n_digits * 2 * poly);
  std::optional<SeedArgs> sa;
  drained(c, [&] { // the arguments are pageable; the scratch returns to the pool drained
    // the randomness keys, the sampled residues and their NTT forms do not stay behind in pool memory the next call reuses
    Wipe w_rk{c, rk.d, (size_t)32 * n_digits}, w_sm{c, sm.d, sizeof(u64) * n_digits * 3 * poly};
    sa.emplace(c, seeds, n_digits);
    sample_to_ntt(c, n_digits, r1keys, rk.d, 3, 0, c->k, sm.d);
    EW_LAUNCH(k_relin_round1, seeded_grid(c, c->k, n_digits), dim3(256), 0, c->stream, c->dev, sa->s8, sa->buf, sm.d, c->sh->sk.d, share.d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(share_out, share.d, shape.bytes, hipMemcpyDeviceToHost, c->stream));
    w_rk.now();
    w_sm.now();
  });
  c->sh->xfer[4] += (size_t)64 * n_digits;
  c->sh->xfer[5] += shape.bytes;
  API_END
}

// Round 2: this party's share [n_digits][k][N] from the sum of the round-1 shares agg1 [n_digits][2][k][N],
// the round-1 keys again (u_J is regenerated from them, never kept) and fresh keys for (e2, e3).  Launch plan: agg1 and
// both key lists up, NTT(u) from r1keys and NTT(e2), NTT(e3) from r2keys (sample_to_ntt, once per key list), ONE
// k_relin_round2, the share back, the wipes, one drain.
int evah_keygen_relin_round2(evah_ctx *c, uint32_t n_digits, const uint64_t *agg1, const uint8_t *r1keys, const uint8_t *r2keys,
                             uint64_t *share_out) {
  API_BEGIN
  use(c);
  keygen_checks(c);
  const KeyDev shape = key_shape(c, n_digits);
  if (!agg1) throw std::invalid_argument("key pointer is null");
  if (!r1keys || !r2keys) throw std::invalid_argument("randomness key pointer is null");
  if (!share_out) throw std::invalid_argument("output pointer is null");
  keygen_ready(c);
  const size_t poly = (size_t)c->k * c->N;
  Scratch agg(c, (size_t)n_digits * 2 * poly), k1(c, (size_t)4 * n_digits), k2(c, (size_t)4 * n_digits), un(c, (size_t)n_digits * poly),
      en(c, (size_t)n_digits * 2 * poly), share(c, (size_t)n_digits * poly);
  drained(c, [&] { // the arguments are pageable; the scratch returns to the pool drained
    // the randomness keys, the sampled residues and their NTT forms do not stay behind in pool memory the next call reuses
    Wipe w_k1{c, k1.d, (size_t)32 * n_digits}, w_k2{c, k2.d, (size_t)32 * n_digits}, w_un{c, un.d, sizeof(u64) * n_digits * poly},
        w_en{c, en.d, sizeof(u64) * n_digits * 2 * poly};
    HIPCHK(hipMemcpyAsync(agg.d, agg1, shape.bytes, hipMemcpyHostToDevice, c->stream));
    sample_to_ntt(c, n_digits, r1keys, k1.d, 1, 0, c->k, un.d);
    sample_to_ntt(c, n_digits, r2keys, k2.d, 2, 1, c->k, en.d);
    EW_LAUNCH(k_relin_round2, dim3((c->N / 2 + 255) / 256, c->k, n_digits), dim3(256), 0, c->stream, c->dev, agg.d, un.d, en.d, c->sh->sk.d, share.d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(share_out, share.d, shape.bytes / 2, hipMemcpyDeviceToHost, c->stream));
    w_k1.now();
    w_k2.now();
    w_un.now();
    w_en.now();
  });
  c->sh->xfer[4] += shape.bytes + (size_t)64 * n_digits;
  c->sh->xfer[5] += shape.bytes / 2;
  API_END
}

// c0 of an installed relinearization or Galois key -> out [n_digits][k][N]: what a key generated in place
// (evah_keygen_set with c0_out = NULL) owes the host when somebody saves it or uploads it elsewhere
int evah_key_download_c0(evah_ctx *c, int kind, uint32_t galois_elt, uint32_t n_digits, uint64_t *out) {
  API_BEGIN
  use(c);
  if (c->dev.pstep > 1) throw std::invalid_argument("a limb shard holds rows of the keys, not whole keys");
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (kind != EVAH_KEY_RELIN && kind != EVAH_KEY_GALOIS) throw std::invalid_argument("unknown key kind");
  if (!out) throw std::invalid_argument("output pointer is null");
  const KeyDev *kd = nullptr;
  if (kind == EVAH_KEY_RELIN) {
    if (c->sh->relin.d) kd = &c->sh->relin;
  } else {
    auto it = c->sh->galois.find(galois_elt);
    if (it != c->sh->galois.end()) kd = &it->second;
  }
  if (!kd) throw std::invalid_argument("key not present");
  if (kd->rows != c->k) throw std::invalid_argument("a limb shard holds rows of the keys, not whole keys");
  if (n_digits != kd->n_digits) throw std::invalid_argument("invalid key digit count");
  drained(c, [&] { c0_download(c, kd->d, n_digits, out); });
  c->sh->xfer[5] += sizeof(u64) * n_digits * c->k * c->N;
  API_END
}

// `batch` symmetric ciphertexts from c0[b] ([limbs][N] each) and seeds[b] (32 bytes each) as one handle [batch][2][limbs][N]
int evah_ct_upload_seeded_instances(evah_ctx *c, uint32_t batch, uint32_t limbs, double scale, const uint64_t *const *c0,
                                    const uint8_t *const *seeds, int async, evah_ct **out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("host transfers cannot be captured into a graph");
  if (batch < 1 || batch > (uint32_t)KS_BATCH_MAX) throw std::invalid_argument("batch must be 1..64");
  if (limbs < 1 || limbs > c->k - 1) throw std::invalid_argument("invalid limb count for this context");
  if (c->N % 4) throw std::invalid_argument("seeded expansion needs N divisible by 4");
  evah_ct *t = ct_new(c, 2, limbs, scale, batch);
  try {
    for (uint32_t b = 0; b < batch; b++)
      HIPCHK(hipMemcpyAsync(t->d + (size_t)b * 2 * t->ps, c0[b], sizeof(u64) * t->ps, hipMemcpyHostToDevice, c->stream));
    expand_c1(c, t, seeds);
    if (!async) HIPCHK(hipStreamSynchronize(c->stream)); // pageable c0: the caller may reuse it after return
  } catch (...) {
    evah_ct_free(c, t);
    throw;
  }
  count_h2d(c, (sizeof(u64) * t->ps + 32) * batch);
  if (!async) t->buf->ready_everywhere = true;
  *out = t;
  API_END
}

// refill a single 2-polynomial handle (a graph plan's input slot) from c0 and a seed
int evah_ct_write_seeded(evah_ctx *c, evah_ct *ct, const uint64_t *c0, const uint8_t *seed32) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("evah_ct_write_seeded cannot be captured into a graph");
  if (ct->size != 2 || ct->batch != 1) throw std::invalid_argument("a seeded write needs a single ciphertext of size 2");
  if (ct->ps != (size_t)ct->limbs * c->N) throw std::invalid_argument("cannot write into a mod-switched view");
  acquire(c, ct->buf);
  HIPCHK(hipMemcpyAsync(ct->d, c0, sizeof(u64) * ct->ps, hipMemcpyHostToDevice, c->stream));
  expand_c1(c, ct, &seed32);
  HIPCHK(hipStreamSynchronize(c->stream));
  count_h2d(c, sizeof(u64) * ct->ps + 32);
  API_END
}

// one polynomial of a single ciphertext -> out [limbs][N]: c0 of a seeded value, whose c1 the seed reproduces
int evah_ct_download_poly(evah_ctx *c, const evah_ct *ct, uint32_t poly, uint64_t *out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (ct->batch != 1) throw std::invalid_argument("evah_ct_download_poly takes a single ciphertext");
  if (poly >= ct->size) throw std::invalid_argument("polynomial index out of range");
  acquire(c, ct->buf);
  const size_t row = sizeof(u64) * (size_t)ct->limbs * c->N;
  HIPCHK(hipMemcpyAsync(out, ct->d + poly * ct->ps, row, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  count_d2h(c, row);
  API_END
}

} // extern "C"
