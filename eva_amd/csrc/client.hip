// client.hip — the host-side neighbours of execute() on the device:
// encryption of encoded plaintexts and decryption + decoding of results, i.e. the arithmetic of SEALPublic::encrypt and
// SEALSecret::decrypt (seal.cpp:24-102, 124-146: encoder.encode + encryptor.encrypt; decryptor.decrypt + encoder.decode).
// Each operation is ONE body for up to 64 instances per call, and no launch count depends on the batch; the calls that
// take one handle (evah_encrypt, evah_encrypt_symmetric, evah_decrypt_decode) are the batch of one behind check prologues
// of their own.  Randomness comes from the host (csprng.h) as int8 arrays, or is drawn here from a 32-byte randomness key
// per instance (k_sample_small): same launches, same words.
//   encrypt  : c = (pk0 u + e0, pk1 u + e1) at l+1 limbs, divided-and-rounded by the extra prime
//              (same rule as rescale A.5), plus the plaintext on c0
//   encrypt_symmetric : c1 = a expanded from a 32-byte seed (seeded.hip.h), c0 = pt - (a s + NTT(e)) at pt's limbs
//   decrypt  : m = c0 + c1 s (+ c2 s^2) per limb, inverse transform, exact recomposition to base-2^64
//              words (mixed-radix digits first), the words to one double in SEAL 3.6's order with
//              1/scale folded in and the sign taken against (Q+1)/2, forward special FFT
//              (CKKSEncoder::decode_internal), slot values out.  FP64 with SEAL's operation order and no
//              FMA contraction: the doubles are those of the oracle's evo_decode and of the host
//              decoder, bit for bit (tests/test_decode_parity.py)
//
// The FFT (k_fft_tile): a workgroup keeps 2048 complex points in LDS and runs every stage whose butterflies stay inside
// the tile before it writes.  2048 double2 are 32 KiB: twice that is the whole 64 KiB a kernel may declare statically (no
// room left for the layout below, one workgroup per 64 KiB), while 2048 points already cover every supported N
// (2^10 .. 2^17) in two launches — 11 stages in the contiguous pass, the remaining logN - 11 <= 6 in the strided one —
// and leave room for several workgroups per CU, which a transform of 16 .. 64 tiles per instance needs more than depth.
//   contiguous pass: tile = 2048 consecutive points, the stages with gap 1 .. 1024
//   strided pass   : tile = R = N / 2048 rows (row stride 2048 points) by C = 2048 / R consecutive columns, the stages
//                    with gap 2048 .. N / 2; a row piece is C >= 32 consecutive double2 (512 B), so the accesses coalesce
// The encoder (Gentleman-Sande, gaps ascending) runs contiguous then strided, the decoder (Cooley-Tukey, gaps descending)
// strided then contiguous; N <= 2048 is the contiguous pass alone.
// LDS layout: a double2 fills one of the 16 slots of 16 bytes of a 256-byte bank row, and a ds_read_b128 is served in
// groups of 16 lanes.  Lane bf of a stage with gap 2^s reads element a = bf with a zero bit inserted at position s, so
// for s >= 4 the 16 lanes of a group read 16 consecutive elements, which the linear layout already spreads over the 16
// slots; it is the stages with gap 1 .. 8 that are 2-way in the linear layout, where a and a + 16 fall on one slot.
// Element e lives at e ^ (e >> 4 & 15) ^ (e >> 8): the slot index is the XOR of the three nibbles of e, which moves
// a + 16 to another slot and, being a permutation within each aligned run of 16 elements, keeps the stages with s >= 4
// and the tile's consecutive loads and stores conflict-free.  The XOR stays inside a 256-byte row, so the tile keeps its
// 32 KiB (the padding of DESIGN.md 4 "LDS layout" without its extra words).  This is counted from the access pattern;
// the layout has not been timed against the linear one.

#include "launch.hip.h"
#include "seeded.hip.h"
#include "sampled.hip.h"

namespace evah {

// ---- the tiled FP64 special FFT
constexpr uint32_t FFT_LOG_TILE = 11, FFT_TILE = 1u << FFT_LOG_TILE, FFT_THREADS = 256;

__device__ __forceinline__ uint32_t fft_lds_at(uint32_t e) { return e ^ ((e >> 4) & 15u) ^ (e >> 8); }

// c [batch][N] complex points, instance = blockIdx.y, tile = blockIdx.x; the stages with global gap 2^L for
// L = L0 .. L0 + n_stages - 1, ascending (ENC) or descending (decoder).  lt = log2 points per tile (logN below one tile).
// ENC : k_enc_fft_stage's butterfly (elementwise.hip) with root inv_seq[N - 2 (N >> L + 1) + 1 + g]; the stage
//       L = logN - 1 is k_enc_fft_last's (sum times fix, difference times the pre-scaled root)
// !ENC: DWTHandler::transform_to_rev of SEAL 3.6 (Cooley-Tukey) with root roots[(N >> L + 1) + g]: x = u + v r,
//       y = u - v r, the complex product as four rounded multiplies, a rounded difference and a rounded sum
// g = the butterfly's group in the whole transform = its upper index >> (L + 1).  No FMA contraction in either.
template <bool ENC, bool STRIDED>
__global__ void __launch_bounds__(FFT_THREADS)
k_fft_tile(double2 *c, const double2 *__restrict__ roots, uint32_t logN, uint32_t lt, uint32_t L0, uint32_t n_stages, double2 scaled_root,
           double fix) {
#pragma clang fp contract(off)
  __shared__ double2 tile[FFT_TILE];
  const uint32_t N = 1u << logN, T = 1u << lt, tid = threadIdx.x;
  double2 *x = c + (size_t)blockIdx.y * N;
  const uint32_t logC = STRIDED ? 2 * FFT_LOG_TILE - logN : 0; // columns per strided tile: 2048 / (N / 2048)
  auto global_of = [&](uint32_t e) -> uint32_t {
    if (STRIDED) return ((e >> logC) << FFT_LOG_TILE) + (blockIdx.x << logC) + (e & ((1u << logC) - 1));
    return (blockIdx.x << lt) + e;
  };
  for (uint32_t e = tid; e < T; e += FFT_THREADS) tile[fft_lds_at(e)] = x[global_of(e)];
  __syncthreads();
  for (uint32_t s = 0; s < n_stages; s++) {
    const uint32_t L = ENC ? L0 + s : L0 + n_stages - 1 - s;
    const uint32_t ll = STRIDED ? L - FFT_LOG_TILE + logC : L, gap = 1u << ll; // the gap inside the tile
    const uint32_t groups = N >> (L + 1);
    for (uint32_t bf = tid; bf < (T >> 1); bf += FFT_THREADS) {
      const uint32_t a = ((bf >> ll) << (ll + 1)) + (bf & (gap - 1)), b = a + gap;
      const uint32_t g = global_of(a) >> (L + 1);
      const uint32_t ia = fft_lds_at(a), ib = fft_lds_at(b);
      const double2 u = tile[ia], v = tile[ib];
      if (ENC) {
        if (L + 1 == logN) { // k_enc_fft_last
          tile[ia] = make_double2((u.x + v.x) * fix, (u.y + v.y) * fix);
          const double dx = u.x - v.x, dy = u.y - v.y;
          const double p = dx * scaled_root.x, q = dy * scaled_root.y, sx = dx * scaled_root.y, t = dy * scaled_root.x;
          tile[ib] = make_double2(p - q, sx + t);
        } else { // k_enc_fft_stage
          const double2 r = roots[N - 2 * groups + 1 + g];
          tile[ia] = make_double2(u.x + v.x, u.y + v.y);
          const double dx = u.x - v.x, dy = u.y - v.y;
          const double p = dx * r.x, q = dy * r.y, sx = dx * r.y, t = dy * r.x;
          tile[ib] = make_double2(p - q, sx + t);
        }
      } else {
        const double2 w = roots[groups + g];
        const double ac = v.x * w.x, bd = v.y * w.y, ad = v.x * w.y, bc = v.y * w.x;
        const double tx = ac - bd, ty = ad + bc;
        tile[ia] = make_double2(u.x + tx, u.y + ty);
        tile[ib] = make_double2(u.x - tx, u.y - ty);
      }
    }
    __syncthreads();
  }
  for (uint32_t e = tid; e < T; e += FFT_THREADS) x[global_of(e)] = tile[fft_lds_at(e)];
}

// the special FFT of `batch` instances in c [batch][N]: one launch for N <= 2048, two above
template <bool ENC> static void fft_batched(evah_ctx *c, double2 *cd, const double2 *roots, uint32_t batch, double2 scaled_root, double fix) {
  const uint32_t logN = c->logN;
  if (logN < 10 || logN > 2 * FFT_LOG_TILE - 5) throw std::invalid_argument("the batched client calls need N from 2^10 to 2^17");
  const uint32_t lt = std::min(logN, FFT_LOG_TILE), low = lt, high = logN - lt;
  const dim3 grid(c->N >> lt, batch), block(FFT_THREADS);
  ProfScope ps(c, KC_EW);
  if (ENC || !high) hipLaunchKernelGGL((k_fft_tile<ENC, false>), grid, block, 0, c->stream, cd, roots, logN, lt, 0u, low, scaled_root, fix);
  if (high) hipLaunchKernelGGL((k_fft_tile<ENC, true>), grid, block, 0, c->stream, cd, roots, logN, lt, FFT_LOG_TILE, high, scaled_root, fix);
  if (!ENC && high) hipLaunchKernelGGL((k_fft_tile<ENC, false>), grid, block, 0, c->stream, cd, roots, logN, lt, 0u, low, scaled_root, fix);
  HIPCHK(hipGetLastError());
}

// ---- the encoder of the _many calls: evah_pt_encode's small kernels (elementwise.hip) with an instance index (grid.y)
// Row b of the values lies at byte b * pitch of vals: the call's staged copy of a host array at the tight
// pitch sizeof(T) * n_vals, or the caller's device memory at its own (a torch slice t[:, :n] is pitched).
// T = the type the values arrived in (double, float, uint8_t: evah_encode_encrypt_array); every T converts to
// double exactly, so the slots hold what the double instantiation holds for the converted array.  One scalar load per
// thread: a uint8_t row may start at any byte, and the kernel is bound by its two 16-byte stores per slot, not by the load.
template <class T>
__global__ void __launch_bounds__(256)
k_enc_scatter_rows(const unsigned char *vals, size_t pitch, uint32_t n_vals, const uint32_t *slot_map, double2 *c, uint32_t slots) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= slots) return;
  const double v = (double)reinterpret_cast<const T *>(vals + (size_t)blockIdx.y * pitch)[i % n_vals];
  c += (size_t)blockIdx.y * 2 * slots;
  c[slot_map[i]] = make_double2(v, 0.0);
  c[slot_map[slots + i]] = make_double2(v, -0.0); // conjugate of a real value
}
__global__ void __launch_bounds__(256)
k_enc_round_many(DevCtx cx, const double2 *c, uint32_t limbs, u64 *out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cx.N) return;
  const double t = c[(size_t)blockIdx.y * cx.N + j].x;
  const double x = fabs(t) < 4503599627370496.0 ? round(t) : t; // >= 2^52: already an integer
  const bool neg = signbit(x);
  const u64 mant = (u64)fabs(x); // |x| < 2^63 is guaranteed by the caller's bound
  out += (size_t)blockIdx.y * limbs * cx.N;
  for (uint32_t i = 0; i < limbs; i++) {
    const DevPrime pm = cx.primes[cx.prime_of(i)];
    const u64 r = barrett64(mant, pm.q, pm.brt);
    out[(size_t)i * cx.N + j] = (neg && r) ? pm.q - r : r;
  }
}

// the forward (INVERSE: inverse) transform of n_polys polynomials d [n_polys][limbs][N] in place, under the chain primes
// 0 .. limbs - 1
template <bool INVERSE> static void rows_ntt(evah_ctx *c, u64 *d, uint32_t limbs, uint32_t n_polys) {
  OpPlain::Params p{d, d, (size_t)limbs * c->N, (size_t)limbs * c->N, limbs, 0, 0, {}};
  if (INVERSE) ntt_inverse<OpPlain>(c, p, n_polys * limbs);
  else ntt_forward<OpPlain>(c, p, n_polys * limbs);
}

// ---- the small polynomials: the host's int8 draws, or drawn where they are used (sampled.hip.h)
__global__ void __launch_bounds__(256)
k_small_to_residues(DevCtx cx, const int8_t *small, uint32_t limbs, u64 *out) {
  // out[p][i][n] = small[p][n] mod primes[i] (negative -> q - |v|)
  const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, p = blockIdx.z;
  const int v = small[(size_t)p * cx.N + n];
  const u64 q = cx.primes[cx.prime_of(i)].q;
  out[((size_t)p * limbs + i) * cx.N + n] = v < 0 ? q - (u64)(-v) : (u64)v;
}
// NTT forms [n_polys][limbs][N] of n_polys small polynomials (int8 [n_polys][N] on the device) under the chain primes
// 0 .. limbs - 1, on the calling queue: what the encryptions here and evah_keygen_switch (seeded.hip) make of their draws
void small_to_ntt(evah_ctx *c, const u64 *small8, uint32_t n_polys, uint32_t limbs, u64 *out) {
  EW_LAUNCH(k_small_to_residues, dim3(c->N / 256, limbs, n_polys), dim3(256), 0, c->stream, c->dev, reinterpret_cast<const int8_t *>(small8), limbs, out);
  rows_ntt<false>(c, out, limbs, n_polys);
}
// Polynomials p0 .. p0 + n_polys - 1 of instance inst = blockIdx.y / n_polys from its randomness key rkeys[inst][8],
// straight into residues out [batch][n_polys][limbs][N] under the chain primes 0 .. limbs - 1, k_small_to_residues'
// words (v < 0 ? q - |v| : v).  A workgroup draws SAMPLE_TILE consecutive coefficients — one ChaCha20 block of 8 per
// thread, kept as 8 bytes in LDS — and then writes them limb by limb, thread t the coefficients 2 t, 2 t + 1 (+ 512 r):
// one 16-byte store per lane, 1 KiB contiguous per wave instruction, and no block is computed twice.  N / 8 may be
// below one workgroup (N = 1024: 128 blocks): the idle threads draw nothing and still take part in the stores.
constexpr uint32_t SAMPLE_THREADS = 256, SAMPLE_TILE = 8 * SAMPLE_THREADS;
__global__ void __launch_bounds__(SAMPLE_THREADS)
k_sample_small(DevCtx cx, const uint32_t *__restrict__ rkeys, uint32_t n_polys, uint32_t p0, uint32_t limbs, u64 *out) {
  __shared__ u64 tile8[SAMPLE_THREADS];
  const uint32_t tid = threadIdx.x, inst = blockIdx.y / n_polys, p = p0 + blockIdx.y % n_polys;
  const uint32_t blk = blockIdx.x * SAMPLE_THREADS + tid;
  if (blk < cx.N / 8) {
    uint32_t key[8];
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = rkeys[8 * inst + w];
    tile8[tid] = sampled_block(key, p, blk);
  }
  __syncthreads();
  const int8_t *tile = reinterpret_cast<const int8_t *>(tile8);
  const uint32_t base = blockIdx.x * SAMPLE_TILE, pairs = min(SAMPLE_TILE, cx.N - base) / 2; // N is a multiple of 256
  int v[SAMPLE_TILE / 2 / SAMPLE_THREADS][2];
#pragma unroll
  for (uint32_t r = 0; r < SAMPLE_TILE / 2 / SAMPLE_THREADS; r++) {
    const uint32_t e = tid + r * SAMPLE_THREADS;
    v[r][0] = e < pairs ? tile[2 * e] : 0;
    v[r][1] = e < pairs ? tile[2 * e + 1] : 0;
  }
  u64 *rows = out + (size_t)blockIdx.y * limbs * cx.N + base;
  for (uint32_t i = 0; i < limbs; i++) {
    const u64 q = cx.primes[cx.prime_of(i)].q;
#pragma unroll
    for (uint32_t r = 0; r < SAMPLE_TILE / 2 / SAMPLE_THREADS; r++) {
      const uint32_t e = tid + r * SAMPLE_THREADS;
      if (e < pairs)
        st2(rows + (size_t)i * cx.N + 2 * e, make_ulonglong2(v[r][0] < 0 ? q - (u64)(-v[r][0]) : (u64)v[r][0],
                                                              v[r][1] < 0 ? q - (u64)(-v[r][1]) : (u64)v[r][1]));
    }
  }
}
// the randomness keys [batch][32] (host) into `keys` on the queue, then NTT forms [batch][n_polys][limbs][N] of the
// polynomials p0 .. p0 + n_polys - 1 of every instance: what the int8 copy and small_to_ntt make of the host's draws
// (also evah_keygen_set's and evah_keygen_public's errors, seeded.hip)
void sample_to_ntt(evah_ctx *c, uint32_t batch, const uint8_t *rkeys, u64 *keys, uint32_t n_polys, uint32_t p0, uint32_t limbs, u64 *out) {
  HIPCHK(hipMemcpyAsync(keys, rkeys, (size_t)32 * batch, hipMemcpyHostToDevice, c->stream));
  EW_LAUNCH(k_sample_small, dim3((c->N + SAMPLE_TILE - 1) / SAMPLE_TILE, batch * n_polys), dim3(SAMPLE_THREADS), 0, c->stream, c->dev,
            reinterpret_cast<const uint32_t *>(keys), n_polys, p0, limbs, out);
  rows_ntt<false>(c, out, limbs, batch * n_polys);
}

// ---- the encryptors' kernels
// c[inst][K][i] = pk[K][i] * u[i] + e_K[i], grid.z = 2 inst + K; small = NTT forms [batch][3][up][N] of (u, e0, e1);
// pk [2][k][N]; c [batch][2][up][N]
__global__ void __launch_bounds__(256)
k_encrypt_zero(DevCtx cx, const u64 *pk, const u64 *small, uint32_t up, u64 *c) {
  const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = blockIdx.y, inst = blockIdx.z >> 1, K = blockIdx.z & 1u;
  const DevPrime pm = cx.primes[i];
  small += (size_t)inst * 3 * up * cx.N;
  const u64 u = small[(size_t)i * cx.N + n], e = small[((size_t)(1 + K) * up + i) * cx.N + n];
  const u64 p = pk[((size_t)K * cx.k + i) * cx.N + n];
  c[(((size_t)2 * inst + K) * up + i) * cx.N + n] = addmod(mulmod(p, u, pm), e, pm.q);
}
// c1 = a, c0 = m - (a s + en) for l limbs of instance z (grid.z): m (NTT plaintexts), en (NTT errors) [batch][l][N],
// sk [k][N] by prime, ct [batch][2][l][N]; seeds as k_key_expand takes them
__global__ void __launch_bounds__(256)
k_encrypt_symmetric(DevCtx cx, Seeds8 seeds, const uint32_t *__restrict__ seed_buf, const u64 *m, const u64 *en, const u64 *sk, uint32_t l,
                    u64 *ct) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, z = blockIdx.z;
  if (t >= cx.N / 4 || i >= l) return;
  const uint32_t prime = cx.prime_of(i);
  const DevPrime pm = cx.primes[prime];
  uint32_t key[8];
  seed_words(seeds, seed_buf, z, key);
  u64 a[4], b[4], mv[4], ev[4], sv[4];
  seeded_block(key, prime, t, pm, a);
  const size_t row = (size_t)l * cx.N, off = (size_t)i * cx.N + 4 * (size_t)t, in = z * row + off;
  ld4(m + in, mv);
  ld4(en + in, ev);
  ld4(sk + (size_t)prime * cx.N + 4 * (size_t)t, sv);
#pragma unroll
  for (int r = 0; r < 4; r++) b[r] = submod(mv[r], addmod(mulmod(a[r], sv[r], pm), ev[r], pm.q), pm.q);
  u64 *c0 = ct + (size_t)2 * z * row + off;
  st4(c0 + row, a);
  st4(c0, b);
}

// ---- the decryptor's kernels
// the ciphertexts of a call: separate allocations, possibly views with a polynomial stride of their own
struct DotTab {
  const u64 *ct[KS_BATCH_MAX];
  uint32_t ct_ps[KS_BATCH_MAX]; // poly strides in units of N coefficients
};
// m[inst][i] = c0 + c1 s (+ c2 s^2) of ciphertext inst (grid.z); a size-1 value is its own message
__global__ void __launch_bounds__(256)
k_decrypt_dot(DevCtx cx, DotTab tab, uint32_t size, uint32_t l, const u64 *sk, u64 *m) {
  const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t i = blockIdx.y, inst = blockIdx.z;
  const DevPrime pm = cx.primes[i];
  const size_t off = (size_t)i * cx.N + n, ps = (size_t)tab.ct_ps[inst] * cx.N;
  const u64 *ct = tab.ct[inst];
  const u64 s = sk[off];
  u64 acc = ct[off], sp = s;
  for (uint32_t p = 1; p < size; p++) {
    acc = addmod(acc, mulmod(ct[p * ps + off], sp, pm), pm.q);
    sp = mulmod(sp, s, pm);
  }
  m[(size_t)inst * l * cx.N + off] = acc;
}

// ---- threshold decryption: flooding noise, a party's share, the combination of all shares
// The flooding noise of instance blockIdx.y from its key fkeys[inst][8], as canonical residues out [n][l][N] under the
// chain primes 0 .. l - 1: r = |E| mod q (barrett64: |E| reaches 2^62 while q may have 30 bits), negative -> q - r,
// k_enc_round_many's rule.  The mapping is k_sample_small's: a workgroup draws FLOOD_TILE consecutive coefficients, one
// ChaCha20 block of 8 per thread, parks them in LDS as 8-byte words (16 KiB), and writes them limb by limb, thread t the
// coefficients 2 t, 2 t + 1 (+ 512 r): one 16-byte store per lane, 1 KiB contiguous per wave instruction, no block
// computed twice.  N = 1024 is half a tile: threads 128 .. 255 draw nothing and the stores stop at `pairs`.
// (A thread parks its 64 bytes at stride 64, which the LDS serves with conflicts; that is 4 writes beside a ChaCha20
// block.  Counted, not timed.)
constexpr uint32_t FLOOD_THREADS = 256, FLOOD_TILE = 8 * FLOOD_THREADS;
__global__ void __launch_bounds__(FLOOD_THREADS)
k_sample_flood(DevCtx cx, const uint32_t *__restrict__ fkeys, uint32_t sigma, uint32_t limbs, u64 *out) {
  __shared__ ulonglong2 tile[FLOOD_TILE / 2];
  const uint32_t tid = threadIdx.x, inst = blockIdx.y;
  const uint32_t blk = blockIdx.x * FLOOD_THREADS + tid;
  if (blk < cx.N / 8) {
    uint32_t key[8];
#pragma unroll
    for (int w = 0; w < 8; w++) key[w] = fkeys[8 * inst + w];
    int64_t e[8];
    flood_block(key, sigma, blk, e);
#pragma unroll
    for (int r = 0; r < 4; r++) tile[4 * tid + r] = make_ulonglong2((u64)e[2 * r], (u64)e[2 * r + 1]);
  }
  __syncthreads();
  constexpr uint32_t R = FLOOD_TILE / 2 / FLOOD_THREADS;
  const uint32_t base = blockIdx.x * FLOOD_TILE, pairs = min(FLOOD_TILE, cx.N - base) / 2; // N is a multiple of 512 (the entry point refuses anything else)
  u64 mag[R][2];
  bool neg[R][2];
#pragma unroll
  for (uint32_t r = 0; r < R; r++) {
    const uint32_t e = tid + r * FLOOD_THREADS;
    const ulonglong2 v = e < pairs ? tile[e] : make_ulonglong2(0, 0);
    const int64_t a = (int64_t)v.x, b = (int64_t)v.y;
    neg[r][0] = a < 0;
    neg[r][1] = b < 0;
    mag[r][0] = a < 0 ? (u64)(-a) : (u64)a;
    mag[r][1] = b < 0 ? (u64)(-b) : (u64)b;
  }
  u64 *rows = out + (size_t)inst * limbs * cx.N + base;
  for (uint32_t i = 0; i < limbs; i++) {
    const DevPrime pm = cx.primes[i]; // (as k_decrypt_dot and the two kernels below: a limb shard is refused by the entry points)
#pragma unroll
    for (uint32_t r = 0; r < R; r++) {
      const uint32_t e = tid + r * FLOOD_THREADS;
      if (e < pairs) {
        const u64 x = barrett64(mag[r][0], pm.q, pm.brt), y = barrett64(mag[r][1], pm.q, pm.brt);
        st2(rows + (size_t)i * cx.N + 2 * e, make_ulonglong2(neg[r][0] && x ? pm.q - x : x, neg[r][1] && y ? pm.q - y : y));
      }
    }
  }
}
// h[inst][i] = c1 s + En in place over the noise en [n][l][N] (NTT form), which becomes the share; c1 = polynomial 1 of
// ciphertext inst through the table.  Two coefficients per thread, 16-byte accesses; grid (N / 512, l, n).
__global__ void __launch_bounds__(256)
k_decrypt_share(DevCtx cx, DotTab tab, uint32_t l, const u64 *sk, u64 *en) {
  const size_t n = 2 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x);
  const uint32_t i = blockIdx.y, inst = blockIdx.z;
  const DevPrime pm = cx.primes[i];
  const size_t off = (size_t)i * cx.N + n;
  const ulonglong2 a = ld2(tab.ct[inst] + (size_t)tab.ct_ps[inst] * cx.N + off), s = ld2(sk + off);
  u64 *h = en + (size_t)inst * l * cx.N + off;
  const ulonglong2 e = ld2(h);
  st2(h, make_ulonglong2(addmod(mulmod(a.x, s.x, pm), e.x, pm.q), addmod(mulmod(a.y, s.y, pm), e.y, pm.q)));
}
// m[inst][i] = c0 + sum_p h_p: c0 = polynomial 0 of ciphertext inst through the table, shares[p * n + inst] = instance
// inst of party p's share ([l][N], canonical residues).  One launch whatever the number of parties: the P n pointers lie
// in a buffer of the call.  Two coefficients per thread, 16-byte accesses; grid (N / 512, l, n).
__global__ void __launch_bounds__(256)
k_combine_shares(DevCtx cx, DotTab tab, const u64 *const *__restrict__ shares, uint32_t n_parties, uint32_t l, u64 *m) {
  const size_t n = 2 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x);
  const uint32_t i = blockIdx.y, inst = blockIdx.z, n_inst = gridDim.z;
  const u64 q = cx.primes[i].q;
  const size_t off = (size_t)i * cx.N + n;
  ulonglong2 acc = ld2(tab.ct[inst] + off);
  for (uint32_t p = 0; p < n_parties; p++) {
    const ulonglong2 h = ld2(shares[(size_t)p * n_inst + inst] + off);
    acc.x = addmod(acc.x, h.x, q);
    acc.y = addmod(acc.y, h.y, q);
  }
  st2(m + (size_t)inst * l * cx.N + off, acc);
}

// Garner tables of a level: inv_prefix[i] = (q_0..q_{i-1})^-1 mod q_i, pre_mod[i][t] = q_0..q_{t-1} mod q_i,
// prefix[i][w] = word w of q_0..q_{i-1} (base 2^64, l words), qwords[w] / half[w] = word w of Q / of floor(Q/2)
struct CrtTab {
  const u64 *inv_prefix, *pre_mod, *prefix, *qwords, *half;
};
// the tables in one array of 2 l^2 + 3 l words: [inv_prefix l][pre_mod l*l][prefix l*l][Q l][floor(Q/2) l]
static CrtTab crt_tab_at(const u64 *d, uint32_t l) {
  return CrtTab{d, d + l, d + l + (size_t)l * l, d + l + (size_t)2 * l * l, d + 2 * l + (size_t)2 * l * l};
}
static std::vector<u64> crt_tab_build(const evah_ctx *c, uint32_t l) {
  std::vector<u64> tab((size_t)2 * l * l + 3 * l, 0);
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
// the table `key` of one of the device state's maps, built by build() and uploaded at its first use (freed with the
// context family)
template <class Build> static const u64 *tab_cached(evah_ctx *c, std::map<uint32_t, u64 *> &tabs, uint32_t key, Build build) {
  auto it = tabs.find(key);
  if (it == tabs.end()) {
    const std::vector<u64> tab = build();
    it = tabs.emplace(key, dev_upload<u64>(c, tab.data(), sizeof(u64) * tab.size())).first;
  }
  return it->second;
}
static CrtTab crt_tab_cached(evah_ctx *c, uint32_t l) {
  return crt_tab_at(tab_cached(c, c->sh->crt_tabs, l, [&] { return crt_tab_build(c, l); }), l);
}
// forward roots zeta^br(j) of the decoder's special FFT (hostmath.h), once per context family
static void dec_tables(evah_ctx *c) {
  if (c->sh->dec_roots) return;
  const uint32_t N = c->N;
  const CkksRoots cr = ckks_roots(N);
  std::vector<double> roots(2 * (size_t)N);
  for (uint32_t j = 0; j < N; j++) { roots[2 * j] = cr.fwd[j].real(); roots[2 * j + 1] = cr.fwd[j].imag(); }
  c->sh->dec_roots = dev_upload<double2>(c, roots.data(), sizeof(double2) * N);
}

// Garner's mixed-radix digits v[0 .. l-1] of the residues r of a level-l value, l >= 1: U = sum_i v_i q_0..q_{i-1}.
// LB bounds l.  Up to 16 the loop over the digits is unrolled with the bound as its trip count and the level as a
// uniform predicate, so r[] and v[] are indexed by constants and stay in registers; LB = 62 keeps a loop of l trips over
// arrays that live in scratch memory.  v[i] is not written from l on: its readers carry the same predicate.
// (The shape is the one the register gate of DESIGN.md 1.12 passed: zeroing v[i] inside the loop, or an unroll pragma
// on the inner loop, costs up to 12 VGPRs in the unrolled forms.)
template <int LB> __device__ __forceinline__ void garner(const DevCtx &cx, const CrtTab &t, uint32_t l, const u64 *r, u64 *v) {
  constexpr bool FLAT = LB <= 16;
  constexpr int UNR = FLAT ? LB : 1;
  const int trips = FLAT ? LB : (int)l;
  v[0] = r[0];
#pragma unroll UNR
  for (int i = 1; i < trips; i++)
    if (!FLAT || i < (int)l) {
      const DevPrime pm = cx.primes[i];
      const u64 *pre = t.pre_mod + i * l;
      u128_t acc = {0, 0};
      for (int j = 0; j < i; j++) acc128(acc, v[j] >= pm.q ? barrett64(v[j], pm.q, pm.brt) : v[j], pre[j]);
      v[i] = mulmod(submod(r[i], barrett128(acc, pm), pm.q), t.inv_prefix[i], pm);
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
  garner<62>(cx, t, l, r, v);
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
// one double per decrypted coefficient of instance blockIdx.y, as the real part of the FFT's input
__global__ void __launch_bounds__(256)
k_crt_to_double(DevCtx cx, CrtTab t, uint32_t l, const u64 *coeff, double inv_scale, double2 *out) {
  const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x, inst = blockIdx.y;
  out[inst * cx.N + n] = make_double2(crt_to_double(cx, t, l, coeff + inst * l * cx.N, n, inv_scale), 0.0);
}
// ---- the refresh: the decrypted integer M of a coefficient, divided by 2^t, under the target's primes
// the lift table of (l, L, t) (hostmath.h lift_table_build) as the kernel reads it
struct LiftTab {
  const u64 *half, *wpre, *qmod, *inv2t, *premod;
  u64 qw;
};
// One thread per coefficient n of instance blockIdx.y: coeff [inst][l][N] (the decrypted message, coefficient form) ->
// out [inst][L][N], the canonical residues of M' = floor((M + 2^(t-1)) / 2^t) (t = 0: M), M = U for U <= floor(Q_l / 2),
// else U - Q_l.  Everything is read off the mixed-radix digits v_i of U (garner): the sign by comparing digits with those
// of floor(Q_l / 2) from the top, U mod q_j for a prime j >= l as sum_i v_i (q_0..q_{i-1} mod q_j), and the remainder
// rho = (M + 2^(t-1)) mod 2^t from M mod 2^64 = sum_i v_i (q_0..q_{i-1} mod 2^64) - [neg] (Q_l mod 2^64), wrapping.
// Then M' = (M + 2^(t-1) - rho) / 2^t exactly, i.e. (M_j + (2^(t-1) - rho)) (2^t)^-1 mod q_j: rescale's exact division
// with 2^t in place of a prime.  No multi-word integer is formed.
// LB bounds l, with garner()'s unrolling rule for every loop over the digits here: up to 16, r[] and v[] are indexed by
// constants and stay in registers; the LB = 62 form keeps the loops and the arrays go to scratch memory, as
// crt_to_double's do.
template <int LB>
__global__ void __launch_bounds__(256)
k_refresh_lift(DevCtx cx, CrtTab g, LiftTab t, uint32_t l, uint32_t L, uint32_t sh, const u64 *coeff, u64 *out) {
  constexpr int UNR = LB <= 16 ? LB : 1;
  const size_t n = (size_t)blockIdx.x * blockDim.x + threadIdx.x, inst = blockIdx.y;
  coeff += inst * l * cx.N + n;
  out += inst * L * cx.N + n;
  u64 r[LB], v[LB];
#pragma unroll UNR
  for (int i = 0; i < LB; i++) r[i] = i < (int)l ? coeff[(size_t)i * cx.N] : 0;
  garner<LB>(cx, g, l, r, v);
  bool neg = false, decided = false; // U > floor(Q_l / 2): mixed radix is positional, the first differing digit from the top decides
#pragma unroll UNR
  for (int i = LB - 1; i >= 0; i--)
    if (i < (int)l && !decided && v[i] != t.half[i]) {
      neg = v[i] > t.half[i];
      decided = true;
    }
  int64_t d = 0; // 2^(t-1) - rho, |d| <= 2^61
  if (sh) {
    u64 w = neg ? 0 - t.qw : 0; // M mod 2^64
#pragma unroll UNR
    for (int i = 0; i < LB; i++)
      if (i < (int)l) w += v[i] * t.wpre[i];
    const u64 hb = (u64)1 << (sh - 1), rho = (w + hb) & (((u64)1 << sh) - 1);
    d = (int64_t)hb - (int64_t)rho;
  }
  auto emit = [&](uint32_t j, u64 m) {
    const DevPrime pm = cx.primes[j];
    if (neg) m = submod(m, t.qmod[j], pm.q);
    if (sh) {
      const u64 a = barrett64(d < 0 ? (u64)(-d) : (u64)d, pm.q, pm.brt); // a 30-bit prime is far below |d|
      m = mulmod(addmod(m, d < 0 ? negmod(a, pm.q) : a, pm.q), t.inv2t[j], pm);
    }
    out[(size_t)j * cx.N] = m;
  };
#pragma unroll UNR
  for (int j = 0; j < LB; j++) // a prime the value has a residue of: U mod q_j = r_j
    if (j < (int)l && j < (int)L) emit(j, r[j]);
  for (uint32_t j = l; j < L; j++) {
    const DevPrime pm = cx.primes[j];
    const u64 *pre = t.premod + (size_t)(j - l) * l;
    u128_t acc = {0, 0};
#pragma unroll UNR
    for (int i = 0; i < LB; i++)
      if (i < (int)l) acc128(acc, v[i] >= pm.q ? barrett64(v[i], pm.q, pm.brt) : v[i], pre[i]);
    emit(j, barrett128(acc, pm));
  }
}

// the slot value as the row's type: double as it is; float = the double rounded to nearest-even here, so that half the
// bytes cross to the host; uint8_t = the nearest integer, ties to even, clamped to [0, 255], NaN -> 0
// (np.clip(np.rint(np.nan_to_num(d, nan=0)), 0, 255))
template <class T> __device__ __forceinline__ T dec_value(double x) { return (T)x; }
template <> __device__ __forceinline__ uint8_t dec_value<uint8_t>(double x) {
  const double r = rint(x);
  return r != r ? (uint8_t)0 : (uint8_t)fmin(fmax(r, 0.0), 255.0);
}
// the first n_out slot values of instance blockIdx.y into row blockIdx.y of out, at byte blockIdx.y * pitch (DESIGN.md
// 1.6): the call's scratch at the tight pitch sizeof(T) * n_out, or the caller's device memory at its own
template <class T>
__global__ void __launch_bounds__(256)
k_dec_gather_rows(const double2 *c, const uint32_t *slot_map, uint32_t n_out, uint32_t N, unsigned char *out, size_t pitch) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_out) reinterpret_cast<T *>(out + (size_t)blockIdx.y * pitch)[i] = dec_value<T>(c[(size_t)blockIdx.y * N + slot_map[i]].x);
}

// ---- the device-array calls' own kernel: rows in the caller's device memory, row b at byte b * pitch
// what check_encodable adds up, where the rows are: sums[b] = sum_i |rows[b][i]| as doubles (every T converts exactly).
// One workgroup per row, thread t adds the elements t, t + 256, ... in that order, then a fixed tree through LDS: no
// atomics, so a row gives the same sum on every run.  A NaN or an infinity in the row makes its sum non-finite.
template <class T>
__global__ void __launch_bounds__(256)
k_rows_abs_sum(const unsigned char *rows, size_t pitch, uint32_t n_values, double *sums) {
#pragma clang fp contract(off)
  __shared__ double part[256];
  const uint32_t tid = threadIdx.x;
  const T *row = reinterpret_cast<const T *>(rows + (size_t)blockIdx.x * pitch);
  double s = 0.0;
  for (uint32_t i = tid; i < n_values; i += 256) s += fabs((double)row[i]);
  part[tid] = s;
  __syncthreads();
  for (uint32_t h = 128; h; h >>= 1) {
    if (tid < h) part[tid] += part[tid + h];
    __syncthreads();
  }
  if (!tid) sums[blockIdx.x] = part[0];
}

// ---- one body per operation: no argument checks inside, every entry point below makes its own
// SEAL Encryptor::encrypt of `batch` NTT-form plaintexts pt [batch][l][N] (a handle's words, or the call's scratch) into
// one handle [batch][2][l][N].  Randomness: small = the host's (u ternary, e0, e1 error polynomials) as int8 [batch][3][N], or
// (rkeys) drawn here from a 32-byte key per instance.  Drains the queue: `small` / `rkeys` are pageable host memory —
// unless drain is false (the device-array calls: rkeys is one of the queue's pinned key slots).
static evah_ct *encrypt_public(evah_ctx *c, uint32_t batch, uint32_t l, double scale, const u64 *pt, const int8_t *small,
                               const uint8_t *rkeys, bool drain = true) {
  const uint32_t up = l + 1;
  const size_t N = c->N, B = batch;
  Scratch sm8(c, rkeys ? 4 * B : (3 * B * N + 7) / 8), sm(c, 3 * B * up * N), ct(c, 2 * B * up * N), r(c, 2 * B * N);
  evah_ct *o = ct_new(c, 2, l, scale, batch);
  try {
    // drawn here, u, e0, e1 and their keys exist nowhere else: they do not stay behind in pool memory the next call reuses
    Wipe w_keys{c, sm8.d, (size_t)32 * B, !rkeys}, w_sm{c, sm.d, sizeof(u64) * 3 * B * up * N, !rkeys};
    if (rkeys) {
      sample_to_ntt(c, batch, rkeys, sm8.d, 3, 0, up, sm.d);
    } else {
      HIPCHK(hipMemcpyAsync(sm8.d, small, 3 * B * N, hipMemcpyHostToDevice, c->stream));
      small_to_ntt(c, sm8.d, 3 * batch, up, sm.d);
    }
    EW_LAUNCH(k_encrypt_zero, dim3(c->N / 256, up, 2 * batch), dim3(256), 0, c->stream, c->dev, c->sh->pk.d, sm.d, up, ct.d);
    HIPCHK(hipGetLastError());
    // divide and round by prime `l` (the last of the up primes), then add instance b's plaintext to its c0
    OpPlain::Params ip{ct.d + (size_t)l * N, r.d, (size_t)up * N, N, 1, l, 1, {}};
    ntt_inverse<OpPlain>(c, ip, 2 * batch);
    OpModDown::Params mp{r.d, N, ct.d, (size_t)up * N, nullptr, 0, 0, o->d, o->ps, l, l};
    mp.use_add_tab = true;
    for (uint32_t b = 0; b < batch; b++) mp.add_tab.p[2 * b] = pt + b * l * N;
    ntt_forward<OpModDown>(c, mp, 2 * batch * l);
    w_keys.now();
    w_sm.now();
    if (drain) HIPCHK(hipStreamSynchronize(c->stream));
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    evah_ct_free(c, o);
    throw;
  }
  return o;
}

// Encryptor::encrypt_symmetric of `batch` NTT-form plaintexts m [batch][l][N] into one handle: c1 = a from seeds[b],
// c0 = m - (a s + NTT(e)).  e = the host's error polynomials as int8 [batch][N], or (ekeys) drawn here from a 32-byte
// key per instance.  Drains the queue: `e` / `ekeys` and `seeds` are pageable host memory — unless drain is false (the
// device-array calls: ekeys and seeds lie in one of the queue's pinned key slots).
static evah_ct *encrypt_symmetric(evah_ctx *c, uint32_t batch, uint32_t l, double scale, const u64 *m, const int8_t *e,
                                  const uint8_t *ekeys, const uint8_t *seeds, bool drain = true) {
  const size_t N = c->N, B = batch;
  Scratch e8(c, ekeys ? 4 * B : (B * N + 7) / 8), en(c, B * l * N);
  std::optional<SeedArgs> sa; // more than 8 instances: its device buffer returns to the pool after the drain
  evah_ct *o = ct_new(c, 2, l, scale, batch);
  try {
    // the errors (or the keys they are drawn from) do not stay behind in pool memory the next call reuses
    Wipe w_en{c, en.d, sizeof(u64) * B * l * N}, w_e8{c, e8.d, ekeys ? 32 * B : B * N};
    if (ekeys) {
      sample_to_ntt(c, batch, ekeys, e8.d, 1, 1, l, en.d);
    } else {
      HIPCHK(hipMemcpyAsync(e8.d, e, B * N, hipMemcpyHostToDevice, c->stream));
      small_to_ntt(c, e8.d, batch, l, en.d);
    }
    sa.emplace(c, seeds, batch);
    EW_LAUNCH(k_encrypt_symmetric, seeded_grid(c, l, batch), dim3(256), 0, c->stream, c->dev, sa->s8, sa->buf, m, en.d, c->sh->sk.d, l, o->d);
    HIPCHK(hipGetLastError());
    w_en.now();
    w_e8.now();
    if (drain) HIPCHK(hipStreamSynchronize(c->stream));
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    evah_ct_free(c, o);
    throw;
  }
  return o;
}

// bytes per value of a value type of the array calls (EVAH_F64 / EVAH_F32 / EVAH_U8); 0: not a type
static size_t dtype_size(int dtype) { return dtype == EVAH_F64 ? 8 : dtype == EVAH_F32 ? 4 : dtype == EVAH_U8 ? 1 : 0; }
static const char *const VALUE_DTYPE_MSG = "unknown value dtype (EVAH_F64, EVAH_F32 or EVAH_U8)";
// f(T{}) with T = the C++ type of a value type: the one place that maps a dtype to code.  Not a type: VALUE_DTYPE_MSG —
// what encode_many_checks answers; every other site comes behind a dtype check of its entry point.
template <class F> static void with_value_type(int dtype, F f) {
  if (dtype == EVAH_F64) f(double{});
  else if (dtype == EVAH_F32) f(float{});
  else if (dtype == EVAH_U8) f(uint8_t{});
  else throw std::invalid_argument(VALUE_DTYPE_MSG);
}

// host -> device bytes of a client call: the values, its randomness or keys and (symmetric) the seeds
static void count_client_h2d(evah_ctx *c, size_t bytes) { c->sh->xfer[4] += bytes; }

// SEAL Decryptor::decrypt + CKKSEncoder::decode of the n instances that n_handles handles of one size, limb count and
// scale hold together (a single ciphertext is one instance; instance j of a batched handle is d + j * size * ps), read in
// place: the first n_out slot values of each into the rows of `out` as dtype_out, rows in list order, then instance order.
// RowsDst says where the rows are: pitch bytes apart, on the host — the gather writes the call's scratch at the tight
// pitch and a copy follows — or in device memory (evah_decrypt_decode_rows) — the gather writes the
// caller's rows and nothing crosses to the host; wait = false (device rows only) leaves the call in queue order.
// counted: the rows calls add what they bring to the host to the transfer statistics, the handle calls do not.
struct RowsDst { size_t pitch; bool on_device, wait, counted; };
// the instances of a call's handles, acquired, in list order, then instance order
static DotTab dot_tab_of(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles) {
  DotTab tab{};
  for (uint32_t i = 0, r = 0; i < n_handles; i++) {
    acquire(c, cts[i]->buf);
    for (uint32_t j = 0; j < cts[i]->batch; j++, r++) {
      tab.ct[r] = cts[i]->d + (size_t)j * cts[i]->size * cts[i]->ps;
      tab.ct_ps[r] = (uint32_t)(cts[i]->ps / c->N);
    }
  }
  return tab;
}
// the decrypted messages of n instances in coefficient form, m [n][l][N]: the dot product with s and the inverse
// transforms (decrypt_decode and refresh)
static void decrypt_to_coeff(evah_ctx *c, const DotTab &tab, uint32_t size, uint32_t l, uint32_t n, u64 *m) {
  EW_LAUNCH(k_decrypt_dot, dim3(c->N / 256, l, n), dim3(256), 0, c->stream, c->dev, tab, size, l, c->sh->sk.d, m);
  rows_ntt<true>(c, m, l, n);
}
// The decoder behind the messages: front(m) puts the n messages [n][l][N] of scale `scale` on the queue in coefficient
// form — the decryptor's dot product and inverse transforms (decrypt_decode), or the sum of decryption shares
// (decrypt_combine) —, everything behind it is one body: Garner, the FFT, the gather in the row's type,
// the copy, the wipes and the statistics.
template <class Front>
static void decode_messages(evah_ctx *c, uint32_t l, double scale, uint32_t n, uint32_t n_out, int dtype_out, void *out, const RowsDst &rows,
                            Front front) {
  const uint32_t N = c->N;
  enc_tables(c);
  dec_tables(c);
  const CrtTab t = crt_tab_cached(c, l);
  const size_t B = n, row_bytes = dtype_size(dtype_out) * n_out, out_bytes = row_bytes * B;
  const bool to_dev = rows.on_device;
  Scratch m(c, B * l * N), cbuf(c, B * 2 * N), outd(c, to_dev ? 1 : (out_bytes + 7) / 8);
  {
    // the decrypted messages, their FP images and the slot values do not stay behind in pool memory the next call reuses
    Wipe w_m{c, m.d, sizeof(u64) * B * l * N}, w_c{c, cbuf.d, sizeof(double2) * B * N}, w_o{c, outd.d, out_bytes, to_dev};
    front(m.d);
    double2 *cd = reinterpret_cast<double2 *>(cbuf.d);
    EW_LAUNCH(k_crt_to_double, dim3(N / 256, n), dim3(256), 0, c->stream, c->dev, t, l, m.d, 1.0 / scale, cd);
    HIPCHK(hipGetLastError());
    fft_batched<false>(c, cd, c->sh->dec_roots, n, make_double2(0.0, 0.0), 0.0);
    // the one difference between the destinations: the caller's rows, or the scratch at the tight pitch and a copy
    unsigned char *dst = static_cast<unsigned char *>(to_dev ? out : (void *)outd.d);
    const size_t pitch = to_dev ? rows.pitch : row_bytes;
    with_value_type(dtype_out, [&](auto tag) {
      EW_LAUNCH(k_dec_gather_rows<decltype(tag)>, dim3((n_out + 255) / 256, n), dim3(256), 0, c->stream, cd, c->sh->enc_slot_map, n_out, N, dst, pitch);
    });
    HIPCHK(hipGetLastError());
    if (!to_dev && rows.pitch != row_bytes)
      HIPCHK(hipMemcpy2DAsync(out, rows.pitch, outd.d, row_bytes, row_bytes, B, hipMemcpyDeviceToHost, c->stream));
    else if (!to_dev)
      HIPCHK(hipMemcpyAsync(out, outd.d, out_bytes, hipMemcpyDeviceToHost, c->stream));
    w_m.now();
    w_c.now();
    w_o.now();
  }
  if (!to_dev || rows.wait) HIPCHK(hipStreamSynchronize(c->stream));
  if (rows.counted && !to_dev) c->sh->xfer[5] += out_bytes; // device rows: nothing comes to the host
}
// rows = nullptr: out [n][n_out] on the host (the calls that take no pitch)
static void decrypt_decode(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t n, uint32_t n_out, int dtype_out, void *out,
                           const RowsDst *rows = nullptr) {
  const uint32_t l = cts[0]->limbs;
  const RowsDst tight{dtype_size(dtype_out) * n_out, false, true, false};
  decode_messages(c, l, cts[0]->scale, n, n_out, dtype_out, out, rows ? *rows : tight, [&](u64 *m) {
    const DotTab tab = dot_tab_of(c, cts, n_handles);
    decrypt_to_coeff(c, tab, cts[0]->size, l, n, m);
  });
}

// ---- threshold decryption
// is P 2^(sigma + 2) > Q_l ?  (P <= 64, sigma <= 62: the left side is below 2^71.)  A share is refused with P = 1; the
// shares of a handle do not carry sigma, so the rule for P parties is the caller's (client.h combine_shares) to apply.
static bool flood_exceeds_modulus(const evah_ctx *c, uint32_t l, uint32_t parties, uint32_t sigma) {
  u128 Q = 1;
  for (uint32_t i = 0; i < l; i++) {
    if (Q >> 64) return false; // Q_l >= 2^64 2^29 already
    Q *= c->primes[i];
  }
  return ((u128)parties << (sigma + 2)) > Q;
}
// evah_decrypt_share_handles: the share h = c1 s + NTT(E) of every instance of the handles, E drawn here from fkeys
// [n][32], into one handle [n][1][l][N].  Launches: the key copy, k_sample_flood, the forward transform of the n l rows,
// k_decrypt_share, the wipe of the keys, one drain — their number does not depend on n.
static evah_ct *decrypt_share(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t n, uint32_t sigma, const uint8_t *fkeys) {
  const uint32_t l = cts[0]->limbs;
  const size_t B = n;
  const DotTab tab = dot_tab_of(c, cts, n_handles);
  Scratch keys(c, 4 * B);
  evah_ct *o = ct_new(c, 1, l, cts[0]->scale, n);
  try {
    Wipe w_keys{c, keys.d, 32 * B}; // whoever learns E learns c1 s: the keys do not stay behind in pool memory
    HIPCHK(hipMemcpyAsync(keys.d, fkeys, 32 * B, hipMemcpyHostToDevice, c->stream));
    EW_LAUNCH(k_sample_flood, dim3((c->N + FLOOD_TILE - 1) / FLOOD_TILE, n), dim3(FLOOD_THREADS), 0, c->stream, c->dev,
              reinterpret_cast<const uint32_t *>(keys.d), sigma, l, o->d);
    HIPCHK(hipGetLastError());
    rows_ntt<false>(c, o->d, l, n);
    EW_LAUNCH(k_decrypt_share, dim3(c->N / 512, l, n), dim3(256), 0, c->stream, c->dev, tab, l, c->sh->sk.d, o->d);
    HIPCHK(hipGetLastError());
    w_keys.now();
    HIPCHK(hipStreamSynchronize(c->stream)); // `fkeys` is pageable host memory
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    evah_ct_free(c, o);
    throw;
  }
  count_client_h2d(c, 32 * B); // the keys: what the call sends up
  return o;
}
// evah_decrypt_combine_rows: decode_messages behind m = c0 + sum_p h_p.  The P n share pointers cross in one copy on the
// queue into a buffer of the call (a launch's arguments cannot hold 64 x 64 of them); the copy of pageable memory
// returns once the words are staged, so the table may leave with this scope.
static void decrypt_combine(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t n, const evah_ct *const *shares,
                            uint32_t n_parties, uint32_t n_out, int dtype_out, void *out, const RowsDst *rows) {
  const uint32_t l = cts[0]->limbs;
  std::vector<const u64 *> ptrs((size_t)n_parties * n);
  Scratch pd(c, ptrs.size());
  decode_messages(c, l, cts[0]->scale, n, n_out, dtype_out, out, *rows, [&](u64 *m) {
    const DotTab tab = dot_tab_of(c, cts, n_handles);
    for (uint32_t p = 0; p < n_parties; p++) {
      acquire(c, shares[p]->buf);
      for (uint32_t j = 0; j < n; j++) ptrs[(size_t)p * n + j] = shares[p]->d + (size_t)j * shares[p]->size * shares[p]->ps;
    }
    HIPCHK(hipMemcpyAsync(pd.d, ptrs.data(), sizeof(u64 *) * ptrs.size(), hipMemcpyHostToDevice, c->stream));
    EW_LAUNCH(k_combine_shares, dim3(c->N / 512, l, n), dim3(256), 0, c->stream, c->dev, tab, reinterpret_cast<const u64 *const *>(pd.d), n_parties, l,
              m);
    HIPCHK(hipGetLastError());
    rows_ntt<true>(c, m, l, n);
  });
}

// ---- the _many calls: values in, one batched handle out
// the checks both encryption calls share, in the order evah_pt_encode and the encryptors make them
static void encode_shape_checks(evah_ctx *c, uint32_t batch, const void *values, uint32_t n_values, uint32_t limbs, const void *out) {
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (batch < 1 || batch > (uint32_t)KS_BATCH_MAX) throw std::invalid_argument("batch must be 1..64");
  if (!values) throw std::invalid_argument("value pointer is null");
  if (!out) throw std::invalid_argument("output pointer is null");
  if (limbs < 1 || limbs > c->k - 1) throw std::invalid_argument("invalid limb count for this context");
  const uint32_t slots = c->N >> 1;
  if (n_values < 1 || n_values > slots || slots % n_values) throw std::invalid_argument("value count must divide the slot count");
  if (c->N % 256) throw std::invalid_argument("encryption needs N divisible by 256");
}
static void encode_many_checks(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs, double scale,
                               const void *out) {
  encode_shape_checks(c, batch, values, n_values, limbs, out);
  // evah_pt_encode's: "encoded values are too large", on the values in the type they came in (the verdict on their
  // float64 image: the conversion is exact, and a float NaN or infinity is a double NaN or infinity)
  with_value_type(dtype, [&](auto tag) { check_encodable(c, static_cast<const decltype(tag) *>(values), batch, n_values, scale); });
}
// values [batch][n_values] of `dtype` (host) -> NTT-form plaintexts pt [batch][limbs][N] on the queue; vals, cbuf: the
// call's scratch.  The values cross in their own type and become doubles in the scatter.
// dev (the device-array calls): `values` is the caller's device memory with dev->pitch bytes between rows —
// nothing is copied, the scatter reads it in place, and dev->release(), right behind the scatter, hands the array back to
// the stream that produced it.
struct DevSrc {
  size_t pitch;
  void *producer;         // the stream that wrote the array, as the ABI names it; NULL: the caller synchronised beforehand
  bool host_wait = false; // set by release(): no producer stream to hand back to, the call waits for dev_out on the host
  void release(evah_ctx *c);
};
static void encode_many(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs, double scale, u64 *vals,
                        double2 *cd, u64 *pt, DevSrc *dev = nullptr) {
  const uint32_t N = c->N, slots = N >> 1;
  enc_tables(c);
  // the one difference between the sources: a host array is copied first and read at the tight pitch
  const size_t pitch = dev ? dev->pitch : dtype_size(dtype) * n_values;
  if (!dev) HIPCHK(hipMemcpyAsync(vals, values, pitch * batch, hipMemcpyHostToDevice, c->stream));
  const unsigned char *src = static_cast<const unsigned char *>(dev ? values : vals);
  with_value_type(dtype, [&](auto tag) {
    EW_LAUNCH(k_enc_scatter_rows<decltype(tag)>, dim3((slots + 255) / 256, batch), dim3(256), 0, c->stream, src, pitch, n_values, c->sh->enc_slot_map, cd, slots);
  });
  HIPCHK(hipGetLastError());
  if (dev) dev->release(c);
  const double fix = scale / (double)N;
  fft_batched<true>(c, cd, c->sh->enc_roots, batch, make_double2(c->sh->enc_last_root[0] * fix, c->sh->enc_last_root[1] * fix), fix);
  EW_LAUNCH(k_enc_round_many, dim3((N + 255) / 256, batch), dim3(256), 0, c->stream, c->dev, cd, limbs, pt);
  HIPCHK(hipGetLastError());
  rows_ntt<false>(c, pt, limbs, batch);
}
// evah_encode_encrypt_many (small: the host's draws), evah_encode_encrypt_sampled_many (rkeys: drawn here) and
// evah_encode_encrypt_array (rkeys, values of `dtype`)
static void encode_encrypt_many(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs, double scale,
                                const int8_t *small, const uint8_t *rkeys, evah_ct **out) {
  use(c);
  encode_many_checks(c, batch, values, dtype, n_values, limbs, scale, out);
  if (!small && !rkeys) throw std::invalid_argument("randomness pointer is null");
  if (!c->sh->pk.d) throw std::invalid_argument("public key not present");
  if (limbs + 1 > c->k) throw std::invalid_argument("plaintext level is not valid for encryption");
  const size_t N = c->N, B = batch;
  Scratch vals(c, (dtype_size(dtype) * B * n_values + 7) / 8), cbuf(c, B * 2 * N), pt(c, B * limbs * N);
  try {
    encode_many(c, batch, values, dtype, n_values, limbs, scale, vals.d, reinterpret_cast<double2 *>(cbuf.d), pt.d);
    *out = encrypt_public(c, batch, limbs, scale, pt.d, small, rkeys);
  } catch (...) {
    (void)hipStreamSynchronize(c->stream); // `values` is pageable host memory
    throw;
  }
  count_client_h2d(c, dtype_size(dtype) * B * n_values + (rkeys ? 32 * B : 3 * B * N));
}

// evah_encode_encrypt_symmetric_many (e: the host's draws), evah_encode_encrypt_symmetric_sampled_many (ekeys: drawn here)
// and evah_encode_encrypt_symmetric_array (ekeys, values of `dtype`)
static void encode_encrypt_symmetric_many(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs,
                                          double scale, const int8_t *e, const uint8_t *ekeys, const uint8_t *seeds, evah_ct **out) {
  use(c);
  encode_many_checks(c, batch, values, dtype, n_values, limbs, scale, out);
  if (!c->sh->sk.d) throw std::invalid_argument("secret key not present");
  if ((!e && !ekeys) || !seeds) throw std::invalid_argument("error polynomial and seed are required");
  const size_t N = c->N, B = batch;
  Scratch vals(c, (dtype_size(dtype) * B * n_values + 7) / 8), cbuf(c, B * 2 * N), pt(c, B * limbs * N);
  try {
    encode_many(c, batch, values, dtype, n_values, limbs, scale, vals.d, reinterpret_cast<double2 *>(cbuf.d), pt.d);
    *out = encrypt_symmetric(c, batch, limbs, scale, pt.d, e, ekeys, seeds);
  } catch (...) {
    (void)hipStreamSynchronize(c->stream); // `values` is pageable host memory
    throw;
  }
  count_client_h2d(c, dtype_size(dtype) * B * n_values + (ekeys ? 32 * B : B * N) + 32 * B);
}

// evah_pt_encode_array and its stream-ordered form: the encoder of the _many calls with the plaintexts
// kept — instance b of the handle is evah_pt_encode of row b's float64 image, word for word.  The launches are
// encode_many's, so their number does not depend on the batch.  wait: drain the queue (`values` is pageable host
// memory); otherwise the copy stays in queue order and the caller keeps `values` until the queue is synchronised.
static void pt_encode_array(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs, double scale, bool wait,
                            evah_pt **out) {
  use(c);
  encode_many_checks(c, batch, values, dtype, n_values, limbs, scale, out);
  const size_t N = c->N, B = batch;
  Scratch vals(c, (dtype_size(dtype) * B * n_values + 7) / 8), cbuf(c, B * 2 * N);
  evah_pt *t = pt_new(c, limbs, scale, batch);
  try {
    encode_many(c, batch, values, dtype, n_values, limbs, scale, vals.d, reinterpret_cast<double2 *>(cbuf.d), t->d);
    if (wait) HIPCHK(hipStreamSynchronize(c->stream));
  } catch (...) {
    (void)hipStreamSynchronize(c->stream); // `values` is pageable host memory
    evah_pt_free(c, t);
    throw;
  }
  if (wait) t->buf->ready_everywhere = true;
  count_client_h2d(c, dtype_size(dtype) * B * n_values);
  *out = t;
}

// ---- the device-array calls: the same bodies with the rows in the caller's device memory
// an event of the queue, made at first use (never while capturing: these calls refuse a capturing context first)
static hipEvent_t cached_event(hipEvent_t &e) {
  if (!e) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return e;
}
// the stream the ABI names: hipStreamLegacy is the null stream
static hipStream_t producer_stream(void *producer) { return (hipStream_t)producer == hipStreamLegacy ? nullptr : (hipStream_t)producer; }
// before the first read of the caller's array: the queue waits for what its producer has enqueued so far
static void wait_for_producer(evah_ctx *c, void *producer) {
  if (!producer) return;
  hipEvent_t e = cached_event(c->dev_in);
  HIPCHK(hipEventRecord(e, producer_stream(producer)));
  HIPCHK(hipStreamWaitEvent(c->stream, e, 0));
}
// behind the last kernel that reads it: whatever the producer enqueues next (an overwrite, a free and reuse) waits for the read
void DevSrc::release(evah_ctx *c) {
  hipEvent_t e = cached_event(c->dev_out);
  HIPCHK(hipEventRecord(e, c->stream));
  if (producer) HIPCHK(hipStreamWaitEvent(producer_stream(producer), e, 0));
  else host_wait = true;
}
// `p` .. `p + span` must be device memory of the context's GPU: asked of the runtime, before anything is launched
static void check_device_rows(evah_ctx *c, const void *p, size_t span, const std::string &what) {
  hipPointerAttribute_t at{};
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) (void)hipGetLastError(); // (a pointer the runtime has never seen: plain host memory)
  if (e != hipSuccess || at.type == hipMemoryTypeUnregistered || at.type == hipMemoryTypeHost)
    throw std::invalid_argument(what + " is host memory: this call takes device memory (use the host-array call, or copy the array to the GPU)");
  if (at.type == hipMemoryTypeManaged || at.isManaged)
    throw std::invalid_argument(what + " is managed memory: this call takes device memory (hipMalloc, or a torch tensor on the GPU)");
  if (at.type != hipMemoryTypeDevice) throw std::invalid_argument(what + " is not device memory");
  if (at.device != c->device)
    throw std::invalid_argument(what + " is memory of GPU " + std::to_string(at.device) + ", this context runs on GPU " + std::to_string(c->device));
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void *>(p)) != hipSuccess) {
    (void)hipGetLastError(); // (an allocator the runtime keeps no range for: the caller's shape is taken as given)
    return;
  }
  const uintptr_t lo = (uintptr_t)base, at_p = (uintptr_t)p;
  if (at_p < lo || span > size || at_p - lo > size - span) throw std::invalid_argument(what + ": the rows run past the end of their allocation");
}
// the shape of rows in device memory: item size of `dtype`, pitch, alignment, and where the memory lives
static void check_rows_shape(evah_ctx *c, const void *p, int dtype, const char *dtype_msg, size_t n_rows, size_t n_cols, size_t pitch, bool on_device,
                             const std::string &what) {
  const size_t item = dtype_size(dtype);
  if (!item) throw std::invalid_argument(dtype_msg);
  if (pitch < item * n_cols) throw std::invalid_argument("row pitch is smaller than a row");
  if (pitch % item) throw std::invalid_argument("row pitch is not a multiple of the item size");
  if ((uintptr_t)p % item) throw std::invalid_argument(what + " is not aligned to its item size");
  if (on_device) check_device_rows(c, p, (n_rows - 1) * pitch + item * n_cols, what);
}
// sums[b] = k_rows_abs_sum of row b, brought to the host: one launch, one copy of 8 * rows bytes, one wait
static void rows_abs_sum(evah_ctx *c, uint32_t rows, const void *values, int dtype, size_t pitch, uint32_t n_values, double *sums) {
  Scratch sd(c, rows);
  const unsigned char *v = static_cast<const unsigned char *>(values);
  double *d = reinterpret_cast<double *>(sd.d);
  with_value_type(dtype, [&](auto tag) { EW_LAUNCH(k_rows_abs_sum<decltype(tag)>, dim3(rows), dim3(256), 0, c->stream, v, pitch, n_values, d); });
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(sums, d, sizeof(double) * rows, hipMemcpyDeviceToHost, c->stream);
  const hipError_t s = hipStreamSynchronize(c->stream); // also on an error: the scratch returns to the pool behind the launch
  HIPCHK(e);
  HIPCHK(s);
  c->sh->xfer[5] += sizeof(double) * rows;
}
// check_encodable's rule on a row's sum of absolute values; a NaN or an infinity in the row left the sum non-finite
static void check_row_sums(const evah_ctx *c, const double *sums, uint32_t batch, uint32_t n_values, double scale) {
  const uint32_t slots = c->N >> 1;
  for (uint32_t b = 0; b < batch; b++) {
    const double bound = 2.0 * sums[b] * (double)(slots / n_values) * scale / (double)c->N;
    if (!std::isfinite(sums[b]) || !(bound < 4611686018427387904.0)) throw std::invalid_argument("encoded values are too large"); // 2^62
  }
}

// a pinned block for the randomness keys (and seeds) of one call: the copies that read it are asynchronous, and the slot
// is taken again only after the event recorded behind them.  Slots whose copies have finished are zeroed as soon as a
// later call looks: the keys are secrets.
static evah_ctx::KeySlot &key_slot(evah_ctx *c) {
  for (auto &s : c->key_slots)
    if (s.busy && hipEventQuery(s.done) == hipSuccess) {
      std::memset(s.host, 0, evah_ctx::KEY_SLOT_BYTES);
      s.busy = false;
    }
  (void)hipGetLastError(); // (hipErrorNotReady of a query is not an error)
  evah_ctx::KeySlot &s = c->key_slots[c->key_slot_next];
  c->key_slot_next = (c->key_slot_next + 1) % evah_ctx::KEY_SLOTS;
  if (!s.host) HIPCHK(hipHostMalloc(reinterpret_cast<void **>(&s.host), evah_ctx::KEY_SLOT_BYTES, hipHostMallocDefault));
  if (s.busy) {
    HIPCHK(hipEventSynchronize(s.done));
    s.busy = false;
  }
  cached_event(s.done);
  return s;
}

// evah_encode_encrypt_array_dev (rkeys) and evah_encode_encrypt_symmetric_array_dev (ekeys, seeds): the bodies of
// encode_encrypt_many / encode_encrypt_symmetric_many with the rows read where they are.  No drain: the handle is valid
// in queue order.  On an error the queue is drained, so no read of `values` is pending when the call returns.
static void encode_encrypt_dev(evah_ctx *c, bool symmetric, uint32_t batch, const void *values, int dtype, size_t pitch, void *producer,
                               const double *row_sums, uint32_t n_values, uint32_t limbs, double scale, const uint8_t *keys, const uint8_t *seeds,
                               evah_ct **out) {
  use(c);
  encode_shape_checks(c, batch, values, n_values, limbs, out);
  check_rows_shape(c, values, dtype, VALUE_DTYPE_MSG, batch, n_values, pitch, true, "values");
  if (symmetric) {
    if (!c->sh->sk.d) throw std::invalid_argument("secret key not present");
    if (!keys || !seeds) throw std::invalid_argument("error polynomial and seed are required");
  } else {
    if (!keys) throw std::invalid_argument("randomness pointer is null");
    if (!c->sh->pk.d) throw std::invalid_argument("public key not present");
    if (limbs + 1 > c->k) throw std::invalid_argument("plaintext level is not valid for encryption");
  }
  *out = nullptr;
  wait_for_producer(c, producer);
  std::vector<double> own;
  if (!row_sums) {
    own.resize(batch);
    rows_abs_sum(c, batch, values, dtype, pitch, n_values, own.data());
    row_sums = own.data();
  }
  check_row_sums(c, row_sums, batch, n_values, scale);
  const size_t N = c->N, B = batch;
  evah_ctx::KeySlot &slot = key_slot(c);
  std::memcpy(slot.host, keys, 32 * B);
  if (symmetric) std::memcpy(slot.host + 32 * KS_BATCH_MAX, seeds, 32 * B);
  slot.busy = true; // from here on the slot holds keys: zeroed behind its event, whatever happens
  DevSrc src{pitch, producer};
  try {
    Scratch cbuf(c, B * 2 * N), pt(c, B * limbs * N);
    encode_many(c, batch, values, dtype, n_values, limbs, scale, nullptr, reinterpret_cast<double2 *>(cbuf.d), pt.d, &src);
    *out = symmetric ? encrypt_symmetric(c, batch, limbs, scale, pt.d, nullptr, slot.host, slot.host + 32 * KS_BATCH_MAX, false)
                     : encrypt_public(c, batch, limbs, scale, pt.d, nullptr, slot.host, false);
    HIPCHK(hipEventRecord(slot.done, c->stream));
    if (src.host_wait) HIPCHK(hipEventSynchronize(c->dev_out));
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    std::memset(slot.host, 0, evah_ctx::KEY_SLOT_BYTES);
    slot.busy = false;
    if (*out) { evah_ct_free(c, *out); *out = nullptr; }
    throw;
  }
  count_client_h2d(c, (symmetric ? 64 : 32) * B);
}

// ---- the refresh
// the lift table of (l, L, t) on the device, built once per context family (freed with it)
static LiftTab lift_tab_cached(evah_ctx *c, uint32_t l, uint32_t L, uint32_t t) {
  const u64 *d = tab_cached(c, c->sh->lift_tabs, l | L << 8 | t << 16, [&] { return lift_table_build(c->primes, l, L, t); });
  const LiftLayout at{l, L};
  // (Q_l mod 2^64 travels as an argument: wrapping products of the chain primes, as the builder forms them)
  u64 qw = 1;
  for (uint32_t i = 0; i < l; i++) qw *= c->primes[i];
  return LiftTab{d + at.half(), d + at.wpre(), d + at.qmod(), d + at.inv2t(), d + at.premod(), qw};
}
template <int LB>
static void launch_refresh_lift(evah_ctx *c, const CrtTab &g, const LiftTab &t, uint32_t l, uint32_t L, uint32_t sh, uint32_t n, const u64 *m,
                                u64 *out) {
  EW_LAUNCH(k_refresh_lift<LB>, dim3(c->N / 256, n), dim3(256), 0, c->stream, c->dev, g, t, l, L, sh, m, out);
}
// evah_refresh_handles: the n instances of the handles (one size, l limbs, scale 2^a) decrypted, their integer messages
// divided by 2^sh and encrypted again at L limbs and scale_out into one handle [n][2][L][N].  The launches are those of
// decrypt_decode up to the inverse transforms, k_refresh_lift, one forward transform of the n L rows, and the tail of
// encrypt_symmetric: their number does not depend on n.  One drain of the queue, at the end.
static evah_ct *refresh(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t n, uint32_t L, uint32_t sh, double scale_out,
                        const uint8_t *ekeys, const uint8_t *seeds) {
  const uint32_t l = cts[0]->limbs;
  const size_t N = c->N, B = n;
  const CrtTab g = crt_tab_cached(c, l);
  const LiftTab t = lift_tab_cached(c, l, L, sh);
  const DotTab tab = dot_tab_of(c, cts, n_handles);
  Scratch m(c, B * l * N), mo(c, B * L * N);
  evah_ct *o = nullptr;
  try {
    // the decrypted messages, at both levels, do not stay behind in pool memory the next call reuses
    Wipe w_m{c, m.d, sizeof(u64) * B * l * N}, w_mo{c, mo.d, sizeof(u64) * B * L * N};
    decrypt_to_coeff(c, tab, cts[0]->size, l, n, m.d);
    if (l <= 2) launch_refresh_lift<2>(c, g, t, l, L, sh, n, m.d, mo.d);
    else if (l <= 4) launch_refresh_lift<4>(c, g, t, l, L, sh, n, m.d, mo.d);
    else if (l <= 8) launch_refresh_lift<8>(c, g, t, l, L, sh, n, m.d, mo.d);
    else if (l <= 16) launch_refresh_lift<16>(c, g, t, l, L, sh, n, m.d, mo.d);
    else launch_refresh_lift<62>(c, g, t, l, L, sh, n, m.d, mo.d);
    HIPCHK(hipGetLastError());
    w_m.now();
    rows_ntt<false>(c, mo.d, L, n);
    o = encrypt_symmetric(c, n, L, scale_out, mo.d, nullptr, ekeys, seeds, false);
    w_mo.now();
    HIPCHK(hipStreamSynchronize(c->stream)); // `ekeys` and `seeds` are pageable host memory
  } catch (...) {
    (void)hipStreamSynchronize(c->stream);
    if (o) evah_ct_free(c, o);
    throw;
  }
  count_client_h2d(c, 64 * B);
  return o;
}

} // namespace evah

extern "C" {

int evah_pt_encode_array(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs, double scale,
                         evah_pt **out) {
  API_BEGIN
  pt_encode_array(c, batch, values, dtype, n_values, limbs, scale, true, out);
  API_END
}

int evah_pt_encode_array_async(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs, double scale,
                               evah_pt **out) {
  API_BEGIN
  pt_encode_array(c, batch, values, dtype, n_values, limbs, scale, false, out);
  API_END
}

// the public key [2][k][N] / the secret key in NTT form [k][N] (client side), resident like the other keys
int evah_client_key_upload(evah_ctx *c, int kind, const uint64_t *data) {
  API_BEGIN
  use(c);
  if (kind != EVAH_KEY_PUBLIC && kind != EVAH_KEY_SECRET) throw std::invalid_argument("unknown key kind");
  KeyDev shape;
  shape.n_digits = 1;
  shape.bytes = sizeof(u64) * (size_t)(kind == EVAH_KEY_PUBLIC ? 2 : 1) * c->k * c->N;
  KeyAlloc key(c, shape, false); // (no split copy: these are no key-switching keys) freed again if the upload fails
  h2d_now(c, key.kd.d, data, key.kd.bytes);
  KeyDev &slot = kind == EVAH_KEY_PUBLIC ? c->sh->pk : c->sh->sk;
  if (slot.d) {
    if (kind == EVAH_KEY_SECRET) (void)hipMemset(slot.d, 0, slot.bytes); // no key material in freed HBM
    (void)hipFree(slot.d);
  }
  slot = key.release();
  API_END
}

// SEAL Encryptor::encrypt of an NTT-form plaintext with the caller's randomness: small = (u ternary,
// e0, e1 error polynomials) as int8 [3][N]
int evah_encrypt(evah_ctx *c, const evah_pt *pt, const int8_t *small, evah_ct **out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (!c->sh->pk.d) throw std::invalid_argument("public key not present");
  if (pt->batch != 1) throw std::invalid_argument("encrypt takes a single plaintext (a batch is encrypted by the evah_encode_encrypt_* calls)");
  acquire(c, pt->buf);
  if (pt->limbs + 1 > c->k) throw std::invalid_argument("plaintext level is not valid for encryption");
  *out = encrypt_public(c, 1, pt->limbs, pt->scale, pt->d, small, nullptr);
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
  if (pt->limbs < 1 || pt->limbs > c->k - 1) throw std::invalid_argument("plaintext level is not valid for encryption"); // no special prime
  if (pt->batch != 1) throw std::invalid_argument("encrypt takes a single plaintext (a batch is encrypted by the evah_encode_encrypt_* calls)");
  acquire(c, pt->buf);
  *out = encrypt_symmetric(c, 1, pt->limbs, pt->scale, pt->d, e, nullptr, seed32);
  API_END
}

int evah_encode_encrypt_many(evah_ctx *c, uint32_t batch, const double *values, uint32_t n_values, uint32_t limbs, double scale,
                             const int8_t *small, evah_ct **out) {
  API_BEGIN
  encode_encrypt_many(c, batch, values, EVAH_F64, n_values, limbs, scale, small, nullptr, out);
  API_END
}

int evah_encode_encrypt_sampled_many(evah_ctx *c, uint32_t batch, const double *values, uint32_t n_values, uint32_t limbs, double scale,
                                     const uint8_t *rkeys, evah_ct **out) {
  API_BEGIN
  encode_encrypt_many(c, batch, values, EVAH_F64, n_values, limbs, scale, nullptr, rkeys, out);
  API_END
}

int evah_encode_encrypt_symmetric_many(evah_ctx *c, uint32_t batch, const double *values, uint32_t n_values, uint32_t limbs, double scale,
                                       const int8_t *e, const uint8_t *seeds, evah_ct **out) {
  API_BEGIN
  encode_encrypt_symmetric_many(c, batch, values, EVAH_F64, n_values, limbs, scale, e, nullptr, seeds, out);
  API_END
}

int evah_encode_encrypt_symmetric_sampled_many(evah_ctx *c, uint32_t batch, const double *values, uint32_t n_values, uint32_t limbs,
                                               double scale, const uint8_t *ekeys, const uint8_t *seeds, evah_ct **out) {
  API_BEGIN
  encode_encrypt_symmetric_many(c, batch, values, EVAH_F64, n_values, limbs, scale, nullptr, ekeys, seeds, out);
  API_END
}

// the two sampled calls on an array in its own type: the same bodies, the values converted in the scatter
int evah_encode_encrypt_array(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs, double scale,
                              const uint8_t *rkeys, evah_ct **out) {
  API_BEGIN
  encode_encrypt_many(c, batch, values, dtype, n_values, limbs, scale, nullptr, rkeys, out);
  API_END
}

int evah_encode_encrypt_symmetric_array(evah_ctx *c, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs,
                                        double scale, const uint8_t *ekeys, const uint8_t *seeds, evah_ct **out) {
  API_BEGIN
  encode_encrypt_symmetric_many(c, batch, values, dtype, n_values, limbs, scale, nullptr, ekeys, seeds, out);
  API_END
}

// SEAL Decryptor::decrypt + CKKSEncoder::decode: the first n_out slot values of the message of ct
int evah_decrypt_decode(evah_ctx *c, const evah_ct *ct, uint32_t n_out, double *out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (!c->sh->sk.d) throw std::invalid_argument("secret key not present");
  if (ct->batch != 1) throw std::invalid_argument("decrypt takes a single ciphertext");
  if (n_out < 1 || n_out > c->N >> 1) throw std::invalid_argument("slot count out of range");
  if (ct->limbs > 61) throw std::invalid_argument("too many limbs");
  check_scale(c, ct->scale, ct->limbs); // decode_internal: "scale out of bounds"
  decrypt_decode(c, &ct, 1, 1, n_out, EVAH_F64, out);
  API_END
}

int evah_decrypt_decode_many(evah_ctx *c, const evah_ct *const *cts, uint32_t n, uint32_t n_out, double *out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (!c->sh->sk.d) throw std::invalid_argument("secret key not present");
  if (n < 1 || n > (uint32_t)KS_BATCH_MAX) throw std::invalid_argument("batch must be 1..64");
  if (!cts || !out) throw std::invalid_argument("ciphertext list and output are required");
  for (uint32_t i = 0; i < n; i++) {
    const std::string at = "ciphertext " + std::to_string(i);
    if (!cts[i]) throw std::invalid_argument(at + " is null");
    if (cts[i]->batch != 1) throw std::invalid_argument(at + ": decrypt takes a single ciphertext");
    if (cts[i]->size != cts[0]->size) throw std::invalid_argument(at + ": size differs from ciphertext 0");
    if (cts[i]->limbs != cts[0]->limbs) throw std::invalid_argument(at + ": limb count differs from ciphertext 0");
    if (cts[i]->scale != cts[0]->scale) throw std::invalid_argument(at + ": scale differs from ciphertext 0");
  }
  if (cts[0]->size < 1 || cts[0]->size > 3) throw std::invalid_argument("ciphertext size out of range");
  if (n_out < 1 || n_out > c->N >> 1) throw std::invalid_argument("slot count out of range");
  if (cts[0]->limbs > 61) throw std::invalid_argument("too many limbs");
  if (c->N % 256) throw std::invalid_argument("decryption needs N divisible by 256");
  check_scale(c, cts[0]->scale, cts[0]->limbs); // decode_internal: "scale out of bounds"
  decrypt_decode(c, cts, n, n, n_out, EVAH_F64, out);
  API_END
}

// evah_decrypt_decode_many over handles that may be batched: the same checks in the same order, the
// instances counted over the whole list
// the checks of evah_decrypt_decode_handles before and behind its dtype check (evah_decrypt_decode_rows makes the same)
// need_sk = false: evah_decrypt_combine_rows, the one reader of ciphertexts here that uses no secret key
static uint32_t handles_checks_list(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, const void *out, bool need_sk = true) {
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (need_sk && !c->sh->sk.d) throw std::invalid_argument("secret key not present");
  if (n_handles < 1) throw std::invalid_argument("batch must be 1..64");
  if (!cts || !out) throw std::invalid_argument("ciphertext list and output are required");
  uint64_t n = 0;
  for (uint32_t i = 0; i < n_handles; i++) {
    const std::string at = "ciphertext " + std::to_string(i);
    if (!cts[i]) throw std::invalid_argument(at + " is null");
    if (cts[i]->size != cts[0]->size) throw std::invalid_argument(at + ": size differs from ciphertext 0");
    if (cts[i]->limbs != cts[0]->limbs) throw std::invalid_argument(at + ": limb count differs from ciphertext 0");
    if (cts[i]->scale != cts[0]->scale) throw std::invalid_argument(at + ": scale differs from ciphertext 0");
    n += cts[i]->batch;
  }
  if (n > (uint64_t)KS_BATCH_MAX) throw std::invalid_argument("the handles hold more than 64 instances in total");
  return (uint32_t)n;
}
static void handles_checks_shape(evah_ctx *c, const evah_ct *const *cts, uint32_t n_out) {
  if (cts[0]->size < 1 || cts[0]->size > 3) throw std::invalid_argument("ciphertext size out of range");
  if (n_out < 1 || n_out > c->N >> 1) throw std::invalid_argument("slot count out of range");
  if (cts[0]->limbs > 61) throw std::invalid_argument("too many limbs");
  if (c->N % 256) throw std::invalid_argument("decryption needs N divisible by 256");
  check_scale(c, cts[0]->scale, cts[0]->limbs); // decode_internal: "scale out of bounds"
}

int evah_decrypt_decode_handles(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t n_out, int dtype_out, void *out) {
  API_BEGIN
  use(c);
  const uint32_t n = handles_checks_list(c, cts, n_handles, out);
  if (dtype_out != EVAH_F64 && dtype_out != EVAH_F32) throw std::invalid_argument("unknown output dtype (EVAH_F64 or EVAH_F32)");
  handles_checks_shape(c, cts, n_out);
  decrypt_decode(c, cts, n_handles, n, n_out, dtype_out, out);
  API_END
}

// ---- the device-array calls
int evah_rows_abs_sum_dev(evah_ctx *c, uint32_t rows, const void *values, int dtype, size_t row_pitch, void *producer, uint32_t n_values,
                          double *sums_out) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("this call synchronises with the host and cannot be captured into a graph");
  if (rows < 1) throw std::invalid_argument("row count must be at least 1");
  if (!values) throw std::invalid_argument("value pointer is null");
  if (!sums_out) throw std::invalid_argument("output pointer is null");
  if (n_values < 1) throw std::invalid_argument("value count must be at least 1");
  check_rows_shape(c, values, dtype, VALUE_DTYPE_MSG, rows, n_values, row_pitch, true, "values");
  wait_for_producer(c, producer);
  rows_abs_sum(c, rows, values, dtype, row_pitch, n_values, sums_out); // (waits: the read is over, nothing to hand back)
  API_END
}

int evah_encode_encrypt_array_dev(evah_ctx *c, uint32_t batch, const void *values, int dtype, size_t row_pitch, void *producer,
                                  const double *row_sums, uint32_t n_values, uint32_t limbs, double scale, const uint8_t *rkeys, evah_ct **out) {
  API_BEGIN
  encode_encrypt_dev(c, false, batch, values, dtype, row_pitch, producer, row_sums, n_values, limbs, scale, rkeys, nullptr, out);
  API_END
}

int evah_encode_encrypt_symmetric_array_dev(evah_ctx *c, uint32_t batch, const void *values, int dtype, size_t row_pitch, void *producer,
                                            const double *row_sums, uint32_t n_values, uint32_t limbs, double scale, const uint8_t *ekeys,
                                            const uint8_t *seeds, evah_ct **out) {
  API_BEGIN
  encode_encrypt_dev(c, true, batch, values, dtype, row_pitch, producer, row_sums, n_values, limbs, scale, ekeys, seeds, out);
  API_END
}

int evah_decrypt_decode_rows(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t n_out, int dtype_out, void *out,
                             size_t row_pitch, int out_on_device, int wait) {
  API_BEGIN
  use(c);
  const uint32_t n = handles_checks_list(c, cts, n_handles, out);
  if (!dtype_size(dtype_out)) throw std::invalid_argument("unknown output dtype (EVAH_F64, EVAH_F32 or EVAH_U8)");
  handles_checks_shape(c, cts, n_out);
  check_rows_shape(c, out, dtype_out, "unknown output dtype (EVAH_F64, EVAH_F32 or EVAH_U8)", n, n_out, row_pitch, out_on_device != 0, "out");
  const RowsDst rows{row_pitch, out_on_device != 0, wait != 0, true};
  decrypt_decode(c, cts, n_handles, n, n_out, dtype_out, out, &rows);
  API_END
}

// ---- threshold decryption
int evah_decrypt_share_handles(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t smudge_bits, const uint8_t *fkeys,
                               evah_ct **out) {
  API_BEGIN
  use(c);
  if (c->dev.pstep > 1) throw std::invalid_argument("a limb shard holds no whole secret key");
  const uint32_t n = handles_checks_list(c, cts, n_handles, out);
  if (!fkeys) throw std::invalid_argument("flooding keys are required");
  if (cts[0]->size != 2) throw std::invalid_argument("decryption share expects a size-2 ciphertext (relinearize first)");
  if (cts[0]->limbs < 1 || cts[0]->limbs > c->k - 1) throw std::invalid_argument("invalid limb count for this context");
  if (cts[0]->limbs > 61) throw std::invalid_argument("too many limbs");
  if (c->N % 512) throw std::invalid_argument("decryption needs N divisible by 512");
  if (smudge_bits < 1 || smudge_bits > 62) throw std::invalid_argument("smudge_bits must be 1..62");
  if (flood_exceeds_modulus(c, cts[0]->limbs, 1, smudge_bits)) throw std::invalid_argument("smudge_bits leaves no room at this level");
  *out = decrypt_share(c, cts, n_handles, n, smudge_bits, fkeys);
  API_END
}

int evah_decrypt_combine_rows(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, const evah_ct *const *shares, uint32_t n_parties,
                              uint32_t n_out, int dtype_out, void *out, size_t row_pitch, int out_on_device, int wait) {
  API_BEGIN
  use(c);
  if (c->dev.pstep > 1) throw std::invalid_argument("a limb shard holds no whole ciphertext");
  const uint32_t n = handles_checks_list(c, cts, n_handles, out, false);
  if (cts[0]->size != 2) throw std::invalid_argument("decryption share expects a size-2 ciphertext (relinearize first)");
  if (!shares) throw std::invalid_argument("share list is required");
  if (n_parties < 1 || n_parties > 64) throw std::invalid_argument("the number of parties must be 1..64");
  for (uint32_t p = 0; p < n_parties; p++) {
    const std::string at = "share " + std::to_string(p);
    if (!shares[p]) throw std::invalid_argument(at + " is null");
    if (shares[p]->size != 1) throw std::invalid_argument(at + " is not a decryption share (size 1)");
    if (shares[p]->limbs != cts[0]->limbs) throw std::invalid_argument(at + ": limb count differs from the ciphertexts'");
    if (shares[p]->scale != cts[0]->scale) throw std::invalid_argument(at + ": scale differs from the ciphertexts'");
    if (shares[p]->batch != n) throw std::invalid_argument(at + ": instance count differs from the ciphertexts'");
  }
  if (!dtype_size(dtype_out)) throw std::invalid_argument("unknown output dtype (EVAH_F64, EVAH_F32 or EVAH_U8)");
  handles_checks_shape(c, cts, n_out);
  if (cts[0]->limbs > c->k - 1) throw std::invalid_argument("invalid limb count for this context");
  if (c->N % 512) throw std::invalid_argument("decryption needs N divisible by 512");
  check_rows_shape(c, out, dtype_out, "unknown output dtype (EVAH_F64, EVAH_F32 or EVAH_U8)", n, n_out, row_pitch, out_on_device != 0, "out");
  const RowsDst rows{row_pitch, out_on_device != 0, wait != 0, true};
  decrypt_combine(c, cts, n_handles, n, shares, n_parties, n_out, dtype_out, out, &rows);
  API_END
}

// ---- the refresh
// the exponent of a scale 2^a, a an integer
static int pow2_exponent(double scale) {
  int e = 0;
  if (!(scale > 0) || !std::isfinite(scale) || std::frexp(scale, &e) != 0.5)
    throw std::invalid_argument("scale is not a power of two: refresh takes scales 2^a with a an integer");
  return e - 1;
}

int evah_refresh_handles(evah_ctx *c, const evah_ct *const *cts, uint32_t n_handles, uint32_t limbs_out, double scale_out, const uint8_t *ekeys,
                         const uint8_t *seeds, evah_ct **out) {
  API_BEGIN
  use(c);
  if (c->dev.pstep > 1) throw std::invalid_argument("a limb shard holds no whole secret key");
  const uint32_t n = handles_checks_list(c, cts, n_handles, out);
  if (!ekeys || !seeds) throw std::invalid_argument("error polynomial and seed are required");
  if (cts[0]->size < 1 || cts[0]->size > 3) throw std::invalid_argument("ciphertext size out of range");
  if (cts[0]->limbs > 61) throw std::invalid_argument("too many limbs");
  if (limbs_out < 1 || limbs_out > c->k - 1 || cts[0]->limbs < 1 || cts[0]->limbs > c->k - 1)
    throw std::invalid_argument("invalid limb count for this context");
  const int t = pow2_exponent(cts[0]->scale) - pow2_exponent(scale_out);
  if (t < 0) throw std::invalid_argument("the target scale is above the value's: refresh divides, it does not multiply");
  if (t > 62) throw std::invalid_argument("the scale ratio exceeds 2^62");
  if (c->N % 256) throw std::invalid_argument("refresh needs N divisible by 256");
  *out = refresh(c, cts, n_handles, n, limbs_out, (uint32_t)t, scale_out, ekeys, seeds);
  API_END
}

} // extern "C"
