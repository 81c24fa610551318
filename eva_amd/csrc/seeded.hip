// seeded.hip — ciphertexts whose second polynomial travels as a 32-byte seed (SEAL's Encryptor::encrypt_symmetric
// followed by a seeded save): uploads of c0 + seed with c1 expanded on the queue (the expansion rule:
// seeded.hip.h), slot refills of captured graphs, and the download of c0 alone.  The fused symmetric encryption
// (evah_encrypt_symmetric) lives in client.hip beside evah_encrypt.

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
  u64 *row = dst + z * inst_stride + (size_t)i * cx.N + 4 * (size_t)t;
  st2(row, make_ulonglong2(a[0], a[1]));
  st2(row + 2, make_ulonglong2(a[2], a[3]));
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

} // namespace evah

extern "C" {

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
