/*
 * eva_hip.h — C-ABI of libeva_hip.so: the MI355X (gfx950) CKKS evaluation backend that
 * replaces the SEAL Evaluator calls behind EVA's execute() path.
 *
 * Each entry point names the reference interface it replaces (paths relative to
 * /root/reference).  Conventions:
 *   - every function returns 0 on success, non-zero on error; evah_last_error() gives the
 *     message (the reference throws C++ exceptions: seal_executor.h:130,146,171,402 and SEAL's
 *     invalid_argument / logic_error; the host wrapper rethrows std::runtime_error).
 *   - handles are opaque; device memory is owned by the backend; uploads and downloads copy.
 *   - a ciphertext is `size` polynomials x `limbs` RNS limbs x N uint64 residues in NTT form,
 *     poly-major / limb-major / coefficient-contiguous (SEAL's layout); limb i is mod primes[i].
 *     limbs = (k-1) - level, where level is EVA's EncodeAtLevelAttribute / signature level
 *     (seal_executor.h:221-224, seal.cpp:59-62).
 *   - one evah_ctx is driven from one host thread at a time; distinct contexts are independent.
 */
#ifndef EVA_HIP_H
#define EVA_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct evah_ctx evah_ctx; /* replaces seal::SEALContext + seal::Evaluator (seal.h:58-66) */
typedef struct evah_ct evah_ct;   /* replaces seal::Ciphertext in SEALExecutor::Objects (seal_executor.h:32-42) */
typedef struct evah_pt evah_pt;   /* replaces seal::Plaintext  in SEALExecutor::Objects */
typedef struct evah_graph evah_graph; /* a captured execute(): replaces re-walking the DAG per call */

/* Last error message of the calling thread ("" if none). */
const char *evah_last_error(void);
/* ABI version of this header. */
int evah_abi_version(void);
/* Number of visible HIP devices. */
int evah_device_count(int *count);

/* ---- context -------------------------------------------------------------------------------
 * Replaces getSEALContext(params) + seal::Evaluator(context) (seal.cpp:148-172, seal.h:52).
 * primes: the key-level chain in CoeffModulus::Create order, special prime last (seal.cpp:181).
 * The backend derives psi (minimal primitive 2N-th root) and all NTT tables itself. */
int evah_ctx_create(uint32_t poly_degree, uint32_t n_primes, const uint64_t *primes, int device,
                    evah_ctx **out);
/* A second issue queue on the same device state: shares the parent's tables and keys (uploaded
 * through either), owns its own HIP stream and buffer pool.  Independent DAG nodes / independent
 * programs issued through different forks overlap on the GPU — the stream-level counterpart of
 * the reference's Galois worker threads (multicore_program_traversal.h:55-78).  A handle may be
 * read by any fork once the producing fork has been synchronised.  Values produced through a
 * fork live in that fork's pool: free them before destroying it (values it only read may outlive it). */
int evah_ctx_fork(evah_ctx *parent, evah_ctx **out);
void evah_ctx_destroy(evah_ctx *ctx);
/* Launch on an external HIP stream (hipStream_t as void*); NULL restores the context's own. */
int evah_ctx_set_stream(evah_ctx *ctx, void *hip_stream);
/* Block until all work issued on the context's stream has finished. */
int evah_ctx_sync(evah_ctx *ctx);
/* *busy = 1 while work enqueued on this queue has not finished (hipStreamQuery), without waiting: how the host side of
 * execute() (seal.cpp:104-122) notices that the caller issued a call while the previous one is still running (r6: twin
 * graph plans) */
int evah_ctx_busy(evah_ctx *ctx, int *busy);
/* Bytes currently held in the context's device pool (in use + cached). */
int evah_ctx_mem_info(evah_ctx *ctx, size_t *in_use, size_t *cached);

/* ---- keys ----------------------------------------------------------------------------------
 * Replaces the seal::RelinKeys / seal::GaloisKeys members of SEALPublic (seal.h:62-63).
 * data: [n_digits][2][n_primes][N] uint64, NTT form (one size-2 key-level ciphertext per digit;
 * SEAL KSwitchKeys layout).  galois_elt is ignored for the relinearization key.
 * The caller always passes the whole key.  On a context that is a limb shard (evah_ctx_set_shard called
 * BEFORE the upload) only the prime rows that shard multiplies into are kept in HBM — its own data limbs
 * and the special prime — and the context then serves the evah_shard_* entry points only. */
#define EVAH_KEY_RELIN 0
#define EVAH_KEY_GALOIS 1
#define EVAH_KEY_PUBLIC 2 /* evah_client_key_upload */
#define EVAH_KEY_SECRET 3
/* a re-key key TO this context's key pair: evah_key_upload takes it with galois_elt naming a slot (any
 * uint32), keeps it beside the Galois keys and builds the split copy under the same condition; evah_rekey_many applies it.
 * Not seed-compressible (its c1 is no expansion): evah_key_upload_seeded, evah_keygen_switch and evah_keygen_set refuse it. */
#define EVAH_KEY_REKEY 4
int evah_key_upload(evah_ctx *ctx, int kind, uint32_t galois_elt, uint32_t n_digits,
                    const uint64_t *data);
/* The same key from its seed-compressed form (what SEAL's KeyGenerator::create_relin_keys /
 * create_galois_keys hand out as Serializable<RelinKeys / GaloisKeys> objects that are saved seeded): c0 of every digit and
 * the 32-byte seed its c1 is expanded from on ctx's queue — row i of digit J is the expansion rule of the seeded
 * ciphertexts under chain prime i with seed J.  Installs exactly the words evah_key_upload installs for the materialised
 * key (the split copy included), with half of them crossing PCIe; a limb shard copies and expands its own rows only. */
int evah_key_upload_seeded(evah_ctx *ctx, int kind, uint32_t galois_elt, uint32_t n_digits,
                           const uint64_t *c0 /* [n_digits][k][N] */, const uint8_t *seeds /* [n_digits][32] */);
/* The same key generated on the device (KeyGenerator::create_relin_keys / create_galois_keys as the
 * reference calls them in generateKeys, /root/reference/eva/seal/seal.cpp:174-203): the secret key is the one
 * evah_client_key_upload(EVAH_KEY_SECRET) left on ctx, the caller draws what is random — one error polynomial (int8) and
 * one 32-byte seed per digit — and c0 = -(a s + NTT(e)) + [row J] (P mod q_J) s' is formed on ctx's queue with
 * a = the seed's expansion; s' = s^2 (relinearization) or s(X^galois_elt) (Galois) is never stored.  install != 0: the key
 * becomes ctx's, as after evah_key_upload_seeded of the same c0 and seeds.  c0_out != NULL: c0 is copied back, word for
 * word the host generator's compressed key for the same draws.  Not on a limb shard, which holds no whole secret key. */
int evah_keygen_switch(evah_ctx *ctx, int kind, uint32_t galois_elt, uint32_t n_digits,
                       const int8_t *errors /* [n_digits][N] */, const uint8_t *seeds /* [n_digits][32] */,
                       int install, uint64_t *c0_out /* [n_digits][k][N] or NULL */);
/* A whole key set generated on the device from 32-byte randomness keys (every create_relin_keys /
 * create_galois_keys call of generateKeys, seal.cpp:174-203, as one call): key j is the relinearization key
 * (kinds[j] = EVAH_KEY_RELIN, elts[j] ignored) or the Galois key of elts[j], and its digit J is evah_keygen_switch's with
 * errors[J] = sampled_small(ekeys[j][J], 1) (eva_amd/host/csprng.h) and seeds[j][J], word for word, the installed layouts
 * included.  The number of launches does not depend on n_keys; sets whose NTT-form errors exceed EVAH_KEYGEN_SET_WORDS
 * run as chunks of whole keys.  install != 0: every key becomes ctx's; c0_out != NULL: every c0 is copied back.  All or
 * nothing: when anything fails no key of the set is installed.  The error keys are secrets: they cross as a buffer, never
 * as launch arguments, and are zeroed on the queue with everything derived from them.  Refuses what evah_keygen_switch
 * refuses, n_keys == 0, more than 65535 digits in all, and a repeated (kind, element). */
int evah_keygen_set(evah_ctx *ctx, uint32_t n_keys, const int *kinds /* [n_keys] */, const uint32_t *elts /* [n_keys] */,
                    uint32_t n_digits, const uint8_t *ekeys /* [n_keys][n_digits][32] */,
                    const uint8_t *seeds /* [n_keys][n_digits][32] */, int install,
                    uint64_t *c0_out /* [n_keys][n_digits][k][N] or NULL */);
/* The public key generated on the device (KeyGenerator::public_key as generateKeys takes it,
 * seal.cpp:174-203): pk = (-(a s + NTT(e)), a) with a_i = the expansion of seed32 under chain prime i and
 * e = sampled_small(ekey32, 1), from the secret key evah_client_key_upload(EVAH_KEY_SECRET) left on ctx.  install != 0: it
 * becomes ctx's public key, as after evah_client_key_upload(EVAH_KEY_PUBLIC); pk_out != NULL: it is copied back. */
int evah_keygen_public(evah_ctx *ctx, const uint8_t *ekey32, const uint8_t *seed32, int install,
                       uint64_t *pk_out /* [2][k][N] or NULL */);
/* The re-key key from ctx's key pair A to another key pair B of the same parameters, generated on the device from B's
 * PUBLIC key (SEAL has no such call — it is KeyGenerator's key-switching key with a public-key
 * encryption of zero in place of the symmetric one): for digit J and prime row i
 *   d[J][0][i] = pkB0_i u_J + NTT_i(e0_J) + [i == J] (P mod q_J) sA_i,   d[J][1][i] = pkB1_i u_J + NTT_i(e1_J),
 * (u_J, e0_J, e1_J) = sampled_small(rkeys[J], 0 / 1 / 2) (eva_amd/host/csprng.h), sA the secret key
 * evah_client_key_upload(EVAH_KEY_SECRET) left on ctx.  pk_target goes up on ctx's queue into scratch and does not replace
 * ctx's own public key; one launch forms both polynomials of every digit; key_out [n_digits][2][k][N] is the layout
 * evah_key_upload(EVAH_KEY_REKEY) takes on B's side.  The randomness keys are secrets: they, the sampled residues and
 * their NTT forms are zeroed on the queue before their memory returns to the pool, also when the call fails.  Refuses a
 * capturing context, a limb shard, null pointers, a missing secret key, a bad digit count and N not divisible by 256. */
int evah_keygen_rekey(evah_ctx *ctx, const uint64_t *pk_target /* [2][k][N] */, uint32_t n_digits,
                      const uint8_t *rkeys /* [n_digits][32] */, uint64_t *key_out /* [n_digits][2][k][N] */);
/* The two rounds of the collective relinearization-key generation (SEAL has no such call — the protocol
 * of Mouchet et al., "Multiparty homomorphic encryption from ring-learning-with-errors"), for a party whose secret key s
 * evah_client_key_upload(EVAH_KEY_SECRET) left on ctx.  With w_J[i] = [i == J] (P mod q_J), for digit J and prime row i:
 *   round 1:  h0[J][i] = -(a_J[i] u_J[i]) + NTT_i(e0_J) + w_J[i] s[i],   h1[J][i] = a_J[i] s[i] + NTT_i(e1_J),
 *             a_J[i] = the expansion of seeds[J] under chain prime i (never stored), (u_J, e0_J, e1_J) =
 *             sampled_small(r1keys[J], 0 / 1 / 2);
 *   round 2:  g[J][i] = s[i] H0[J][i] + NTT_i(e2_J) + (u_J[i] - s[i]) H1[J][i] + NTT_i(e3_J),  (H0, H1) = agg1[J] the sums of
 *             all parties' round-1 shares, u_J from r1keys[J] again, (e2_J, e3_J) = sampled_small(r2keys[J], 1 / 2).
 * `seeds` are PUBLIC and common to all parties and must not be the seeds of any party's own relinearization key (the
 * caller derives them: relin_round_seed, eva_amd/host/ckks_host.h).  The randomness keys are secrets: they, the sampled
 * residues and their NTT forms are zeroed on the queue before their memory returns to the pool, also when the call
 * fails.  One kernel launch per call after the sampling.  Both refuse what evah_keygen_rekey refuses. */
int evah_keygen_relin_round1(evah_ctx *ctx, uint32_t n_digits, const uint8_t *seeds /* [n_digits][32] */,
                             const uint8_t *r1keys /* [n_digits][32] */, uint64_t *share_out /* [n_digits][2][k][N] */);
int evah_keygen_relin_round2(evah_ctx *ctx, uint32_t n_digits, const uint64_t *agg1 /* [n_digits][2][k][N] */,
                             const uint8_t *r1keys /* [n_digits][32] */, const uint8_t *r2keys /* [n_digits][32] */,
                             uint64_t *share_out /* [n_digits][k][N] */);
/* c0 of an installed relinearization or Galois key (what saving the RelinKeys / GaloisKeys of
 * generateKeys, seal.cpp:174-203, needs of a key that was generated in place): d[J][0] of every digit -> out, one
 * linear copy per digit on ctx's queue, then a drain.  Refuses a key that is not present and a limb shard. */
int evah_key_download_c0(evah_ctx *ctx, int kind, uint32_t galois_elt, uint32_t n_digits,
                         uint64_t *out /* [n_digits][k][N] */);
/* Galois element used by evah_rotate for `steps` (SEAL GaloisTool::get_elt_from_step). */
int evah_galois_elt_from_step(evah_ctx *ctx, int32_t steps, uint32_t *elt);

/* ---- values --------------------------------------------------------------------------------
 * Replace SEALExecutor::setInputs / getOutputs / free (seal_executor.h:264-277,420-435,406-418). */
int evah_ct_upload(evah_ctx *ctx, uint32_t size, uint32_t limbs, double scale,
                   const uint64_t *data /* [size][limbs][N] */, evah_ct **out);
/* ---- pinned host memory for the values setInputs copies in and getOutputs copies out
 * (seal_executor.h:269-270, 420-435; in the reference they live in SEAL's MemoryPool): blocks are
 * page-locked once and recycled by size, so the copies are DMA transfers at PCIe rate.  NULL when
 * no memory can be pinned (no device) — use ordinary memory then.  Thread-safe. */
void *evah_host_alloc(size_t bytes);
void evah_host_free(void *p);

/* ---- batched handles: `batch` (<= 64) independent ciphertexts of one shape in ONE handle
 * ([batch][size][limbs][N]).  Every evaluator entry point above/below accepts them and applies the
 * SEAL call to each instance in one launch set (keys are shared by the instances; a plaintext operand is
 * shared too unless it is a batched plaintext of the same batch, evah_pt_encode_array below; two ciphertext
 * operands must have the same batch).  This is the unit a batch of
 * independent program instances runs on (BASELINE config 4: 256 Sobel DAGs) — the reference runs
 * such a batch as `batch` separate SEALPublic::execute calls (seal.cpp:104-122). */
int evah_ct_upload_batch(evah_ctx *ctx, uint32_t batch, uint32_t size, uint32_t limbs, double scale,
                         const uint64_t *data /* [batch][size][limbs][N] */, evah_ct **out);
/* the same from `batch` separate host arrays, each [size][limbs][N] */
int evah_ct_upload_instances(evah_ctx *ctx, uint32_t batch, uint32_t size, uint32_t limbs, double scale,
                             const uint64_t *const *data, evah_ct **out);
/* every instance of a batched handle into its own host array out[b] ([size][limbs][N] each) */
int evah_ct_download_instances(evah_ctx *ctx, const evah_ct *ct, uint64_t *const *out);
/* Stream-ordered forms of the two calls above, for pipelining a loop of SEALPublic::execute calls
 * (seal.cpp:104-122) over several queues: the copies are enqueued on ctx's queue and the call returns.
 * Host arrays must stay valid and untouched until evah_ctx_sync(ctx); use evah_host_alloc memory for
 * copies that overlap other queues' kernels.  The handle passed to the download may be freed right away. */
int evah_ct_upload_instances_async(evah_ctx *ctx, uint32_t batch, uint32_t size, uint32_t limbs, double scale,
                                   const uint64_t *const *data, evah_ct **out);
int evah_ct_download_instances_async(evah_ctx *ctx, const evah_ct *ct, uint64_t *const *out);
int evah_ct_batch(const evah_ct *ct, uint32_t *batch);
/* n single ciphertexts (same shape, scale) -> one batched handle; device-side copies */
int evah_ct_stack(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n, evah_ct **out);
/* instance b of a batched handle as a single-ciphertext view (shares the buffer; free separately) */
int evah_ct_unstack(evah_ctx *ctx, const evah_ct *ct, uint32_t b, evah_ct **out);
/* instances b0 .. b0 + n - 1 of a batched handle as a batched view of n instances (shares the buffer; free separately):
 * what passes a group of a batch to the evaluator where seal_executor.h:264-277 copies its inputs in.  Mod-switched
 * views and slices can be sliced again; n = 0 or b0 + n > batch is refused. */
int evah_ct_slice(evah_ctx *ctx, const evah_ct *ct, uint32_t b0, uint32_t n, evah_ct **out);

/* a copy of a value owned by another context: another GPU (peer copy over xGMI — the P2P step at the
 * join of independent sub-DAGs) or another issue queue; asynchronous, ordered
 * after the producer of src on its own queue */
int evah_ct_copy(evah_ctx *dst_ctx, const evah_ct *src, evah_ct **out);
int evah_pt_copy(evah_ctx *dst_ctx, const evah_pt *src, evah_pt **out);
/* overwrite an existing handle's residues (same shape) — refills the input slots of a graph */
int evah_ct_write(evah_ctx *ctx, evah_ct *ct, const uint64_t *data);
int evah_pt_write(evah_ctx *ctx, evah_pt *pt, const uint64_t *data);
/* device-to-device refill of an existing handle from another one of the same shape (the input slot of a
 * captured execute() from a device-resident valuation entry: seal_executor.h:264-277 copies inputs in,
 * here without leaving the device); asynchronous on ctx's queue, ordered after the producer of src */
int evah_ct_assign(evah_ctx *ctx, evah_ct *dst, const evah_ct *src);
/* `waiter`'s queue waits for everything enqueued so far on `signaller`'s queue (both of one device
 * state); no host synchronisation.  Orders work the per-buffer tracking cannot see (graph replays). */
int evah_ctx_wait(evah_ctx *waiter, evah_ctx *signaller);
/* values that crossed the host boundary through this context and its forks since creation:
 * out[0] / out[1] = ciphertexts uploaded (evah_ct_upload*, evah_ct_write) / downloaded, out[2] / out[3] =
 * plaintexts uploaded / downloaded, out[4] / out[5] = bytes host->device / device->host of all of them.
 * The valuation of the reference "may hold device handles" (SURVEY.md 8(b)); tests assert that
 * encrypt -> execute -> decrypt moves no ciphertext across. */
int evah_ctx_transfer_stats(evah_ctx *ctx, uint64_t out[6]);
/* the instantiation of the key switch's mod-up kernel this context launches (EVAH_MODUP_LR / EVAH_MODUP_SPEC and the
 * context's primes): out[0] = log2 coefficients per thread (3 or 2), out[1] = 1 when only the top-bit butterflies are
 * compiled in (every prime 2^b - c, b > 32, c < 2^32), out[2] = 1 when only the lazy digit conversion is
 * (q_J <= 8 q_kappa for every digit / output prime pair).  All of them compute the same words. */
int evah_ctx_modup_variant(evah_ctx *ctx, uint32_t out[3]);
/* the tail of relinearize + rescale where its key switch takes the mod-up kernel (EVAH_TAIL_FUSE / EVAH_MODUP_SPEC and
 * the context's primes): out[0] = 1 when it runs as three launches (ntt_tail_kernel), 0 = the six launches; out[1] = 1
 * when that kernel has only the top-bit butterflies compiled in, out[2] = 1 when only the lazy conversion is
 * (q_last <= 4 q_i and P <= 8 q_i for every pair i < last of data primes).  All of them compute the same words. */
int evah_ctx_tail_variant(evah_ctx *ctx, uint32_t out[3]);
/* whether the contiguous passes of that tail run inside the key-switch kernel (EVAH_KS_TAIL: five launches, the key-switch
 * products never stored): out[0] = 1 when this context's relinearize + rescale launch sets take that path — the three-launch
 * tail, the radix-2^30 key switch, every prime of the top-bit shape — at the mod-up kernel's size, on levels of 2 .. 15
 * limbs; out[1] = the fewest workgroups the first key-switch slice (2 n N / 256 for n instances) must have for it, 0 when
 * EVAH_KS_TAIL=1 asks for every such launch set.  Same words either way. */
int evah_ctx_ks_tail(evah_ctx *ctx, uint32_t out[2]);
/* bytes of HBM the evaluation keys (relinearization + Galois + re-key) of this context's device state occupy.  After
 * evah_ctx_set_shard(ctx, s, G) an upload keeps only shard s's prime rows of a key (its data limbs and the
 * special prime): (ceil((k-1)/G) + 1) / k of the whole key. */
int evah_ctx_key_bytes(evah_ctx *ctx, uint64_t *bytes);
/* The same keys with the copies the library keeps beside them (the reference keeps one copy per key, seal.h:58-66):
 * out[0] = the key words as uploaded (= evah_ctx_key_bytes), out[1] = the radix-2^30 split copies of whole keys on
 * contexts whose primes all have the top-bit shape (ks_inner_kernel<MAC3>), out[2] = the permuted copies of Galois
 * keys that hoisted rotation sets have used so far.  Up to 3x out[0]; a copy that does not fit the device is simply
 * not made (the affected launches take the form that does not need it). */
int evah_ctx_key_bytes_detail(evah_ctx *ctx, uint64_t out[3]);
/* Evaluation keys uploaded from the host into ctx's device state so far (the reference uploads nothing: its keys live
 * where SEALPublic lives, seal.h:58-66): out[0] = installed uploads (evah_key_upload, evah_key_upload_seeded), out[1] =
 * the bytes they sent.  A key generated in place (evah_keygen_switch, evah_keygen_set) is not an upload and counts in neither. */
int evah_ctx_key_upload_stats(evah_ctx *ctx, uint64_t out[2]);
/* evah_ct_stack calls made on ctx's device state so far (the deep copies of seal_executor.h:264-277, device to device):
 * out[0] = calls, out[1] = the instances they copied.  A batch passed on as slices of its handles (evah_ct_slice) counts
 * in neither. */
int evah_ctx_stack_stats(evah_ctx *ctx, uint64_t out[2]);
/* Contiguous transform passes that ctx (this queue, not its forks) has launched in the looped form so far: one 64-thread
 * workgroup per 256-coefficient tile that walks several jobs of one prime with the tile's twiddles staged once.  The
 * counters only grow, and count launches made while a graph is captured too.  out[0..3] = launches as inverse pass 1, as
 * plain forward pass 2, as key-switch digit pass 2 and as mod-down pass 2 (the profile classes intt_pass1, ntt_pass2,
 * ksdigit_pass2, moddown_pass2, which the plain form of these passes reports as well); out[4] = the jobs along the
 * launches' loop axes, summed; out[5] = the walks along them, summed (ceil(jobs / jobs per walk) of each launch). */
int evah_ctx_loop_stats(evah_ctx *ctx, uint64_t out[6]);
int evah_ct_info(const evah_ct *ct, uint32_t *size, uint32_t *limbs, double *scale);
int evah_ct_download(evah_ctx *ctx, const evah_ct *ct, uint64_t *out /* [size][limbs][N] */);
void evah_ct_free(evah_ctx *ctx, evah_ct *ct);
/* data in NTT form */
int evah_pt_upload(evah_ctx *ctx, uint32_t limbs, double scale, const uint64_t *data /* [limbs][N] */,
                   evah_pt **out);
/* data in coefficient form (output of the host FP64 encoder); the backend runs the per-limb
 * forward NTT — the device half of CKKSEncoder::encode (seal_executor.h:242). */
int evah_pt_upload_coeff(evah_ctx *ctx, uint32_t limbs, double scale, const uint64_t *data,
                         evah_pt **out);
/* encoder.encode (seal_executor.h:242) entirely on the device: `n_values` reals (replicated over
 * the N/2 slots as seal_executor.h:226-240 does) -> inverse special FFT in FP64 -> round(x*scale/N)
 * -> residues -> NTT.  Bit-identical to the host encoder followed by evah_pt_upload_coeff.  The device
 * keeps |coefficient| in one 64-bit word, so the call refuses, before anything is launched and with SEAL's
 * "encoded values are too large", a non-finite value and an a-priori coefficient bound that reaches 2^62:
 *   bound = 2 * sum |values| * (slots / n_values) * scale / N  (no coefficient exceeds it),  refused unless bound < 2^62.
 * Such encodings take the host's multi-precision path + evah_pt_upload_coeff.  SEAL's own total-modulus
 * rule is not applied here.  The four evah_encode_encrypt_*many calls below make the same check per instance. */
int evah_pt_encode(evah_ctx *ctx, const double *values, uint32_t n_values, uint32_t limbs, double scale, evah_pt **out);
/* plaintext whose every slot is the same residue per limb: encode of a uniform constant
 * (Program::makeUniformConstant, program.h:58-60) — value[i] = round(c*scale) mod primes[i]. */
int evah_pt_uniform(evah_ctx *ctx, uint32_t limbs, double scale, const uint64_t *value /* [limbs] */,
                    evah_pt **out);
int evah_pt_info(const evah_pt *pt, uint32_t *limbs, double *scale);
int evah_pt_download(evah_ctx *ctx, const evah_pt *pt, uint64_t *out /* [limbs][N] */);
void evah_pt_free(evah_ctx *ctx, evah_pt *pt);
/* ---- batched plaintexts: `batch` (<= 64) plaintexts of one level and scale in ONE handle, instance b
 * for instance b of a batched ciphertext of the same batch — the unencrypted input of seal_executor.h:264-277 that
 * differs between the program instances of a batch (a mask, a query, a per-request gain).  evah_add_plain,
 * evah_sub_plain, evah_multiply_plain, evah_weighted_sum (per term), evah_elementwise_program and evah_execute take one
 * wherever they take a plaintext: instance b of the result is the same call on evah_ct_slice(ct, b, 1) and plaintext b.
 * A batch that is neither 1 nor the ciphertext's is refused ("plaintext batch differs from the ciphertext's").
 * evah_rotate_weighted_sums, evah_multiply_plain_many, evah_encrypt, evah_encrypt_symmetric, evah_pt_write and
 * evah_pt_download refuse a batched handle; evah_pt_copy, evah_pt_info and evah_pt_free handle it. */
/* encoder.encode (seal_executor.h:242) of every row of values [batch][n_values] (EVAH_F64 / EVAH_F32 / EVAH_U8, crossing
 * PCIe in that type): instance b = evah_pt_encode of row b converted to double, word for word.  The launches are those
 * of the evah_encode_encrypt_* calls' encoder, their number independent of the batch; checks and messages are theirs
 * (batch 1..64, null pointers, the limb count, n_values dividing the slots, "encoded values are too large" per row, an
 * unknown dtype, a capturing context).  batch = 1 gives an ordinary plaintext.  Bytes sent count in
 * evah_ctx_transfer_stats out[4]. */
int evah_pt_encode_array(evah_ctx *ctx, uint32_t batch, const void *values, int dtype /* EVAH_F64 | EVAH_F32 | EVAH_U8 */,
                         uint32_t n_values, uint32_t limbs, double scale, evah_pt **out);
/* the same, stream-ordered like evah_ct_upload_instances_async: the host -> device copy stays in ctx's queue order and
 * the call returns; `values` must stay valid and untouched until evah_ctx_sync(ctx) */
int evah_pt_encode_array_async(evah_ctx *ctx, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs,
                               double scale, evah_pt **out);
int evah_pt_batch(const evah_pt *pt, uint32_t *batch);
/* every instance of a plaintext handle (batched or single) */
int evah_pt_download_instances(evah_ctx *ctx, const evah_pt *pt, uint64_t *out /* [batch][limbs][N] */);

/* ---- evaluator ops: one per SEAL call made by SEALExecutor::operator() ---------------------- */
/* evaluator.add (seal_executor.h:124); sizes may differ (2/3), limbs and scale must match */
int evah_add(evah_ctx *ctx, const evah_ct *a, const evah_ct *b, evah_ct **out);
/* evaluator.sub (seal_executor.h:140) */
int evah_sub(evah_ctx *ctx, const evah_ct *a, const evah_ct *b, evah_ct **out);
/* evaluator.add_plain (seal_executor.h:127) */
int evah_add_plain(evah_ctx *ctx, const evah_ct *a, const evah_pt *b, evah_ct **out);
/* evaluator.sub_plain (seal_executor.h:143) */
int evah_sub_plain(evah_ctx *ctx, const evah_ct *a, const evah_pt *b, evah_ct **out);
/* evaluator.negate (seal_executor.h:194) */
int evah_negate(evah_ctx *ctx, const evah_ct *a, evah_ct **out);
/* evaluator.multiply, both operands size 2 (seal_executor.h:164) */
int evah_multiply(evah_ctx *ctx, const evah_ct *a, const evah_ct *b, evah_ct **out);
/* n (<= 64) independent evaluator.multiply calls at one level (seal_executor.h:164, once per
 * independent Multiply node / per ciphertext of a batch) issued as ONE launch; outs[i] ==
 * evah_multiply(as[i], bs[i]) bit for bit, the outputs share one allocation */
int evah_multiply_many(evah_ctx *ctx, const evah_ct *const *as, const evah_ct *const *bs, uint32_t n, evah_ct **outs);
/* sum_j cts[j] (*) pts[j] in one pass (pts[j] == NULL: cts[j] itself): the value of the
 * evaluator.multiply_plain (seal_executor.h:168) + evaluator.add (:124) chain a convolution or
 * linear-layer row lowers to; n <= 64 terms of one size, level and product scale */
int evah_weighted_sum(evah_ctx *ctx, const evah_ct *const *cts, const evah_pt *const *pts, uint32_t n, evah_ct **out);
/* evaluator.square, operand size 2 (seal_executor.h:162) */
int evah_square(evah_ctx *ctx, const evah_ct *a, evah_ct **out);
/* evaluator.multiply_plain (seal_executor.h:168) */
int evah_multiply_plain(evah_ctx *ctx, const evah_ct *a, const evah_pt *b, evah_ct **out);
/* n (<= 64) independent multiply_plain calls (seal_executor.h:168) on single ciphertexts of one shape
 * as one launch; outs[i] == evah_multiply_plain(cts[i], pts[i]) */
int evah_multiply_plain_many(evah_ctx *ctx, const evah_ct *const *cts, const evah_pt *const *pts, uint32_t n, evah_ct **outs);
/* evaluator.relinearize, size 3 -> 2 (seal_executor.h:200); needs the relin key */
int evah_relinearize(evah_ctx *ctx, const evah_ct *a, evah_ct **out);
/* evaluator.relinearize immediately followed by evaluator.rescale_to_next (+ scale fix-up) on the
 * result (seal_executor.h:200 then :213-214), evaluated together: identical ciphertext, ~13% fewer
 * transforms.  The host executor uses it when a Relinearize term's only use is a Rescale. */
int evah_relinearize_rescale(evah_ctx *ctx, const evah_ct *a, uint32_t divisor_bits, evah_ct **out);
/* the same for n (<= 64) independent ciphertexts at one level (a batch of multiplications to be
 * relinearized and rescaled): outs[b] == evah_relinearize_rescale(as[b]); one wide launch set,
 * the shared relinearization key is streamed once per XCD for the whole batch. */
int evah_relinearize_rescale_many(evah_ctx *ctx, const evah_ct *const *as, uint32_t n, uint32_t divisor_bits,
                                  evah_ct **outs);
/* evaluator.multiply (seal_executor.h:164), evaluator.relinearize (:200) and
 * evaluator.rescale_to_next + scale fix-up (:213-214) on one pair of size-2 ciphertexts — the
 * Mul -> Relinearize -> Rescale chain every ciphertext product of a compiled CKKS program goes
 * through — evaluated together: the size-3 product is never written to HBM (its polynomials are
 * formed where the key switch and the combine consume them).  Identical ciphertext to the three calls. */
int evah_multiply_relinearize_rescale(evah_ctx *ctx, const evah_ct *a, const evah_ct *b, uint32_t divisor_bits, evah_ct **out);
/* the same for n (<= 64) independent pairs at one level as one launch set; BASELINE.json's
 * op-triple (multiply + relinearize + rescale) is exactly one unit of this call */
int evah_multiply_relinearize_rescale_many(evah_ctx *ctx, const evah_ct *const *as, const evah_ct *const *bs, uint32_t n,
                                           uint32_t divisor_bits, evah_ct **outs);
/* evaluator.multiply (seal_executor.h:164; a == b: evaluator.square, :162), evaluator.rescale_to_next + scale fix-up
 * (:213-214) on the size-3 product and evaluator.relinearize (:200) — the order lazy relinearization
 * (eva/ckks/lazy_relinearizer.h:73-80) gives a product under the waterline rescalers — evaluated together: the
 * size-3 product is never written; the rescaled d2 is formed in coefficient form where the digit decomposition reads it, and
 * the rescale of d0 / d1 shares the forward transform of the key switch's mod-down (six dependent launches).
 * Identical ciphertext to the three calls.  Batched handles: a and b hold the same number of instances, so does *out. */
int evah_multiply_rescale_relinearize(evah_ctx *ctx, const evah_ct *a, const evah_ct *b, uint32_t divisor_bits, evah_ct **out);
/* the same for n independent pairs at one level as one launch set (n x instances per handle <= 64) */
int evah_multiply_rescale_relinearize_many(evah_ctx *ctx, const evah_ct *const *as, const evah_ct *const *bs, uint32_t n,
                                           uint32_t divisor_bits, evah_ct **outs);
/* evaluator.rescale_to_next + scale fix-up (seal_executor.h:213-214) of a size-3 ciphertext followed by evaluator.relinearize
 * (:200): what lazy relinearization (eva/ckks/lazy_relinearizer.h:73-80) leaves after a SUM of products.  Evaluated together
 * like evah_multiply_rescale_relinearize, on the stored polynomials.  Identical ciphertext to the two calls.  Batched handles
 * keep their instance count. */
int evah_rescale_relinearize(evah_ctx *ctx, const evah_ct *a, uint32_t divisor_bits, evah_ct **out);
/* the same for n size-3 ciphertexts at one level as one launch set (n x instances per handle <= 64) */
int evah_rescale_relinearize_many(evah_ctx *ctx, const evah_ct *const *as, uint32_t n, uint32_t divisor_bits, evah_ct **outs);
/* evaluator.rotate_vector(a, steps) (seal_executor.h:181; rightRotate passes -steps, :188);
 * steps == 0 copies; needs the Galois key for exactly this step's element */
int evah_rotate(evah_ctx *ctx, const evah_ct *a, int32_t steps, evah_ct **out);
/* n (<= 64) non-zero rotations of the SAME ciphertext — n evaluator.rotate_vector calls
 * (seal_executor.h:181) issued as one set of n-times-wider launches; outs[r] == evah_rotate(a, steps[r]).
 * The host executor groups the sibling rotations of a term (convolution windows) into one call.
 * Throughput-sized sets are hoisted: c1 is decomposed once and every rotation's key inner product is
 * formed from the permuted digits plus a per-(element, level) constant — the residues are exactly
 * those of rotating first and decomposing after, at 1/n of the transforms.
 * EVAH_HOIST=0 disables, EVAH_HOIST_MIN_TILES sets the size from which it is used. */
int evah_rotate_many(evah_ctx *ctx, const evah_ct *a, const int32_t *steps, uint32_t n, evah_ct **outs);
/* n (<= 64) rotations of SEVERAL ciphertexts of one level, pair i = (cts[i], steps[i] != 0): the
 * sibling rotations of independent sub-expressions (seal_executor.h:181/188 called once per node)
 * as one launch set; outs[i] == evah_rotate(cts[i], steps[i]) bit for bit.  A ciphertext that occurs
 * in several pairs is decomposed once for all of them when the set is large enough (hoisting, as above). */
int evah_rotate_pairs(evah_ctx *ctx, const evah_ct *const *cts, const int32_t *steps, uint32_t n, evah_ct **outs);
/* Re-key: size-2 ciphertexts under another key pair A become ciphertexts under ctx's key pair, with the
 * key evah_key_upload(EVAH_KEY_REKEY, slot) left on ctx — out = (c0 + KS(c1)_0, KS(c1)_1), KS being
 * Evaluator::switch_key_inplace as evah_rotate applies it (seal_executor.h:181 without the permutation), bit for bit;
 * level and scale stay.  cts: single and batched handles, evah_ct_slice / evah_ct_unstack and mod-switched views, of ONE
 * level, read in place — also handles owned by a context of another device state on the same GPU (the read is ordered
 * behind their producer, no copy).  outs[i] holds as many instances as cts[i]; all of them view one allocation.  The
 * instances go out 64 at a time, each chunk one launch set in the form every key switch of that size takes.  Refuses an
 * empty slot ("re-key key not present"), size 3, mixed levels, a handle on another GPU, a limb shard. */
int evah_rekey_many(evah_ctx *ctx, uint32_t slot, const evah_ct *const *cts, uint32_t n_handles, evah_ct **outs);
/* Sums of plaintext-weighted rotations, the convolution pattern of EVA programs
 * (/root/reference/examples/image_processing.py:22-34 convolutionXY: rotated = image << (i*w + j);
 *  Ix += rotated * filter[i][j]; Iy += rotated * filter[j][i]) — the rotate_vector (seal_executor.h:181/188),
 * multiply_plain (:168) and add (:124) calls of every term in one launch set.
 *   window w has win_terms[w] terms (cts / steps, consecutive; steps == 0: the ciphertext itself) and
 *   win_sums[w] sums over those terms; pts holds, window after window, win_sums[w] rows of win_terms[w]
 *   weights (NULL = 1); outs receives the sums of all windows in order:
 *     out = sum_t pts[row][t] (*) rotate(cts[t], steps[t])        — bit for bit the op-by-op result.
 * All ciphertexts: size 2, one level, one batch count; every sum has one product scale (checked as
 * evah_weighted_sum checks it).  Throughput-sized sets whose windows have one or two sums and at most one
 * unrotated term are hoisted AND fused: the rotated ciphertexts are never written — the mod-down's last pass
 * multiplies by the weights and accumulates the sums in registers; other shapes run as
 * evah_rotate_pairs / evah_rotate_many followed by evah_weighted_sum.  EVAH_WIN_FUSE=0 forces the latter. */
int evah_rotate_weighted_sums(evah_ctx *ctx, const evah_ct *const *cts, const int32_t *steps, const uint32_t *win_terms,
                              const uint32_t *win_sums, uint32_t n_windows, const evah_pt *const *pts, evah_ct **outs);
/* n independent evaluator.rescale_to_next calls (seal_executor.h:213) of one size and level,
 * n * size <= 128, as one launch set */
int evah_rescale_many(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n, uint32_t divisor_bits, evah_ct **outs);
/* n (<= 64) independent evaluator.relinearize calls (seal_executor.h:200) of one level as one launch set */
int evah_relinearize_many(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n, evah_ct **outs);
/* evaluator.rescale_to_next + scale fix-up out.scale = a.scale / 2^divisor_bits
 * (seal_executor.h:213-214) */
int evah_rescale(evah_ctx *ctx, const evah_ct *a, uint32_t divisor_bits, evah_ct **out);
/* evaluator.mod_switch_to_next (seal_executor.h:206) */
int evah_mod_switch(evah_ctx *ctx, const evah_ct *a, evah_ct **out);

/* ---- the neighbours of execute() on the device --------------------------
 * SEALPublic::encrypt (seal.cpp:24-102: encoder.encode + encryptor.encrypt) and SEALSecret::decrypt
 * (seal.cpp:124-146: decryptor.decrypt + encoder.decode).  Randomness is the caller's (a host CSPRNG):
 * `small` holds the ternary u and the two error polynomials as int8 [3][N].  Keys: the public key
 * [2][k][N] and the secret key in NTT form [k][N], both uploaded with evah_client_key_upload. */
int evah_client_key_upload(evah_ctx *ctx, int kind /* EVAH_KEY_PUBLIC | EVAH_KEY_SECRET */, const uint64_t *data);
/* (pk0 u + e0, pk1 u + e1) one level above pt, divided-and-rounded by the extra prime, + pt on c0 */
int evah_encrypt(evah_ctx *ctx, const evah_pt *pt, const int8_t *small, evah_ct **out);
/* m = c0 + c1 s (+ c2 s^2) -> inverse transform -> exact recomposition -> double (1/scale folded in) ->
 * special FFT, in the operation order of SEAL 3.6's CKKSEncoder::decode_internal: the first n_out slot
 * values, the same doubles as the host decoder and the CPU oracle produce */
int evah_decrypt_decode(evah_ctx *ctx, const evah_ct *ct, uint32_t n_out, double *out);

/* ---- seeded symmetric ciphertexts (Encryptor::encrypt_symmetric + a seeded save) ---------
 * c1 = a is uniform and travels as a 32-byte seed: limb i, coefficient j is (hi 2^64 + lo) mod q_i with
 * (lo, hi) = u64 words 2 (j % 4), 2 (j % 4) + 1 of the ChaCha20 block with key = seed, block counter j / 4 and
 * nonce 0x6331000000000000 | i.  A ciphertext at a lower level is the prefix of the same expansion.
 * Seeded uploads count in evah_ctx_transfer_stats as c0's words plus 32 bytes per ciphertext. */
/* c1 = a (from seed32), c0 = pt - (a s + NTT(e)) at pt's limbs; e = one error polynomial as int8 [N]; needs
 * EVAH_KEY_SECRET */
int evah_encrypt_symmetric(evah_ctx *ctx, const evah_pt *pt, const int8_t *e, const uint8_t *seed32, evah_ct **out);
/* `batch` size-2 ciphertexts from c0[b] ([limbs][N] each) and seeds[b] (32 bytes each) as one handle; c1 is
 * expanded on ctx's queue.  async = 0: returns when the words have landed; async != 0: stream-ordered like
 * evah_ct_upload_instances_async (c0 arrays stay valid until evah_ctx_sync; the seeds are read at the call) */
int evah_ct_upload_seeded_instances(evah_ctx *ctx, uint32_t batch, uint32_t limbs, double scale, const uint64_t *const *c0,
                                    const uint8_t *const *seeds, int async, evah_ct **out);
/* overwrite a single size-2 handle from c0 [limbs][N] and a seed (the input slot of a captured execute()) */
int evah_ct_write_seeded(evah_ctx *ctx, evah_ct *ct, const uint64_t *c0, const uint8_t *seed32);
/* polynomial `poly` of a single ciphertext -> out [limbs][N] (c0 of a seeded value: its c1 is the seed's) */
int evah_ct_download_poly(evah_ctx *ctx, const evah_ct *ct, uint32_t poly, uint64_t *out);

/* ---- the client calls for a batch per call: what a loop of SEALPublic::encrypt (seal.cpp:24-102:
 * encoder.encode + encryptor.encrypt per input) and of SEALSecret::decrypt (seal.cpp:124-146: decryptor.decrypt +
 * encoder.decode per output) does for the instances of evah_execute's batches, as one launch set whose length does not
 * depend on the batch.  1 <= batch, n <= 64.  One host->device copy per input array, one device->host copy of the
 * result and one drain of ctx's queue per call; the plaintexts exist only in pool scratch.  The encryption calls
 * refuse what evah_pt_encode refuses ("encoded values are too large": a non-finite value or a coefficient bound of
 * 2^62 or more in any instance), before anything is launched. */
/* instance b = evah_pt_encode(values[b]) -> evah_encrypt(small[b]) word for word (seal.cpp:24-102); values
 * [batch][n_values], small int8 [batch][3][N]; out: one batched handle [batch][2][limbs][N] */
int evah_encode_encrypt_many(evah_ctx *ctx, uint32_t batch, const double *values, uint32_t n_values, uint32_t limbs, double scale,
                             const int8_t *small, evah_ct **out);
/* instance b = evah_pt_encode(values[b]) -> evah_encrypt_symmetric(e[b], seeds[b]) word for word (seal.cpp:24-102 with
 * Encryptor::encrypt_symmetric); e int8 [batch][N], seeds [batch][32]; needs EVAH_KEY_SECRET */
int evah_encode_encrypt_symmetric_many(evah_ctx *ctx, uint32_t batch, const double *values, uint32_t n_values, uint32_t limbs,
                                       double scale, const int8_t *e, const uint8_t *seeds, evah_ct **out);
/* The same two calls with the small polynomials drawn on the device in place of the randomness that
 * seal.cpp:85 `encryptor.encrypt` takes from SEAL's generator on the host: a 32-byte randomness key per instance travels
 * instead of 3 N (N) int8 coefficients.  sampled_small(key, p) is the expansion of eva_amd/host/csprng.h.  The keys are
 * secrets: they go up as a pool buffer on ctx's queue, and that buffer, the sampled residues and their NTT forms are
 * zeroed on the queue before they return to the pool, also when the call fails.  Checks, messages, launches per call
 * and the one drain are those of the calls above. */
/* evah_encode_encrypt_many with small[b] = (sampled_small(rkeys[b], 0), sampled_small(rkeys[b], 1),
 * sampled_small(rkeys[b], 2)) word for word (seal.cpp:24-102); rkeys [batch][32] */
int evah_encode_encrypt_sampled_many(evah_ctx *ctx, uint32_t batch, const double *values, uint32_t n_values, uint32_t limbs,
                                     double scale, const uint8_t *rkeys, evah_ct **out);
/* evah_encode_encrypt_symmetric_many with e[b] = sampled_small(ekeys[b], 1) word for word (seal.cpp:24-102 with
 * Encryptor::encrypt_symmetric); ekeys [batch][32] (secret), seeds [batch][32] (public) */
int evah_encode_encrypt_symmetric_sampled_many(evah_ctx *ctx, uint32_t batch, const double *values, uint32_t n_values,
                                               uint32_t limbs, double scale, const uint8_t *ekeys, const uint8_t *seeds,
                                               evah_ct **out);
/* out[i] = the n_out doubles evah_decrypt_decode(cts[i]) returns, bit pattern for bit pattern (seal.cpp:124-146); the n
 * single ciphertexts (views included) share one size, limb count and scale and are read in place; out [n][n_out] */
int evah_decrypt_decode_many(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n, uint32_t n_out, double *out);

/* ---- the client calls on arrays and batched handles -----------------------------------------
 * The inputs of seal.cpp:24-102 arrive as one array [batch][n_values] in the type the caller holds them in, cross PCIe
 * in that type (batch * n_values * itemsize bytes) and become doubles on the device, exactly: the encoder's scatter reads
 * the source type.  Checks, messages, launches per call, wipes and the one drain are those of the _sampled_many calls;
 * "encoded values are too large" is decided on the typed data with the verdict of its float64 image (a float NaN or
 * infinity is refused as the double is).  An unknown dtype is refused. */
#define EVAH_F64 0
#define EVAH_F32 1
#define EVAH_U8 2
/* evah_encode_encrypt_sampled_many on the float64 image of values, word for word (seal.cpp:24-102); values
 * [batch][n_values] of dtype, rkeys [batch][32] */
int evah_encode_encrypt_array(evah_ctx *ctx, uint32_t batch, const void *values, int dtype, uint32_t n_values, uint32_t limbs,
                              double scale, const uint8_t *rkeys, evah_ct **out);
/* evah_encode_encrypt_symmetric_sampled_many on the float64 image of values, word for word (seal.cpp:24-102 with
 * Encryptor::encrypt_symmetric); ekeys [batch][32] (secret), seeds [batch][32] (public) */
int evah_encode_encrypt_symmetric_array(evah_ctx *ctx, uint32_t batch, const void *values, int dtype, uint32_t n_values,
                                        uint32_t limbs, double scale, const uint8_t *ekeys, const uint8_t *seeds, evah_ct **out);
/* evah_decrypt_decode_many (seal.cpp:124-146) over handles that are each single or batched, views and slices included,
 * at most 64 instances together: instance j of a handle is read in place at d + j * size * stride.  out [instances][n_out]
 * of dtype_out, rows in list order, then instance order: EVAH_F64 rows are evah_decrypt_decode_many's bit patterns on the
 * unstacked instances, EVAH_F32 rows are those doubles rounded to nearest-even on the device (half the bytes come back).
 * Refusals and messages are evah_decrypt_decode_many's (mismatches by argument index), plus more than 64 instances in
 * total and an unknown dtype_out. */
int evah_decrypt_decode_handles(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n_handles, uint32_t n_out, int dtype_out,
                                void *out);

/* ---- the array calls on device memory ----------------------------------------------------------
 * The inputs of seal.cpp:24-102 and the outputs of seal.cpp:124-146 as rows that already live in HBM (a torch tensor, an
 * evah_buf): in place of the host -> device copy of evah_encode_encrypt_array and the device -> host copy of
 * evah_decrypt_decode_handles, the encoder's scatter reads and the decoder's gather writes the caller's memory.  Row b
 * starts at byte b * row_pitch of the base; row_pitch is at least a row and a multiple of the item size (a slice
 * t[:, :n] is pitched), the base is aligned to the item size and nothing more.
 * values / out must be device memory of ctx's GPU (hipPointerGetAttributes; host and managed memory are refused by
 * name), and where the runtime knows the allocation the rows must lie inside it.
 * Ordering: ctx's queue is a non-blocking stream and is ordered against nobody else's.  `producer` is the hipStream_t on
 * which the caller's array was written (hipStreamLegacy = (hipStream_t)1 for the null stream), or NULL.  Given, the queue
 * waits for an event recorded on it before its first read, and an event recorded on the queue behind the last kernel
 * that reads `values` is made a dependency of `producer` (hipStreamWaitEvent): a later overwrite, or a free and reuse, on
 * that stream cannot overtake the read.  NULL: the caller has synchronised beforehand, and the call waits on the host
 * for that second event before it returns.  The events are kept by the queue, not created per call.
 * All refusals — a capturing context, memory that is not device memory of this GPU, a pitch smaller than a row or not a
 * multiple of the item size, an unknown dtype, and those of the host-array calls — come before anything is launched. */
/* sums_out[b] (host, `rows` doubles) = sum_i |values[b][i]| in FP64, every value read as the double it converts to
 * exactly: what check_encodable adds up, computed where the rows are.  One launch, one copy of 8 * rows bytes, one wait.
 * A row's sum is the same on every run (fixed order, no atomics) and may differ from a serial sum in its last bits; a
 * NaN or an infinity in a row leaves its sum non-finite.  rows is not limited to 64. */
int evah_rows_abs_sum_dev(evah_ctx *ctx, uint32_t rows, const void *values, int dtype, size_t row_pitch, void *producer,
                          uint32_t n_values, double *sums_out);
/* evah_encode_encrypt_array / evah_encode_encrypt_symmetric_array (seal.cpp:24-102) on rows in device memory: instance b
 * is word for word what those calls give for the same rows brought to the host.  No value byte crosses PCIe; the
 * randomness keys (and seeds) go up as before, through pinned blocks of the queue, and evah_ctx_transfer_stats out[4]
 * grows by 32 * batch (64 * batch).  THE CALL DOES NOT DRAIN THE QUEUE: the handle is valid in queue order, like every
 * evaluator result.
 * row_sums: NULL, and the call computes evah_rows_abs_sum_dev itself (one more launch and one wait); or the sums that
 * evah_rows_abs_sum_dev returned for exactly these rows, to which check_encodable's rule (bound below 2^62, finite) is
 * applied without a launch.  The library TRUSTS such sums: it cannot tell whether the rows were rewritten in between.
 * Sums that understate the rows give wrong words in the affected instances (a coefficient beyond the 63 bits the
 * rounding keeps) — never an access out of bounds: every index the kernels form comes from batch, n_values and
 * row_pitch, not from a value. */
int evah_encode_encrypt_array_dev(evah_ctx *ctx, uint32_t batch, const void *values, int dtype, size_t row_pitch, void *producer,
                                  const double *row_sums, uint32_t n_values, uint32_t limbs, double scale, const uint8_t *rkeys,
                                  evah_ct **out);
int evah_encode_encrypt_symmetric_array_dev(evah_ctx *ctx, uint32_t batch, const void *values, int dtype, size_t row_pitch,
                                            void *producer, const double *row_sums, uint32_t n_values, uint32_t limbs, double scale,
                                            const uint8_t *ekeys, const uint8_t *seeds, evah_ct **out);
/* evah_decrypt_decode_handles (seal.cpp:124-146: the same checks, messages, launches and scratch wipes) into rows of
 * row_pitch bytes.  out_on_device = 0: host memory, and the call waits whatever `wait` says; out_on_device = 1: device
 * memory of ctx's GPU, written by the gather — no device -> host copy — and wait = 0 leaves the call in queue order
 * (evah_ctx_sync, or evah_ctx_wait from the consumer's queue, before the rows are read).  dtype_out: EVAH_F64 and
 * EVAH_F32 rows carry evah_decrypt_decode_handles' bit patterns; EVAH_U8 is the double rounded to the nearest integer,
 * ties to even, clamped to [0, 255], NaN -> 0.  The bytes between rows are not touched.  Host rows count in
 * evah_ctx_transfer_stats out[5], device rows do not. */
int evah_decrypt_decode_rows(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n_handles, uint32_t n_out, int dtype_out, void *out,
                             size_t row_pitch, int out_on_device, int wait);

/* ---- the refresh ---------------------------------------------------------------------------------
 * Decrypt, divide by a power of two and encrypt again under the same secret key, without decoding: the interactive
 * substitute for bootstrapping.  cts: what evah_decrypt_decode_handles takes (single and batched handles, views, slices,
 * mod-switched views, read in place), at most 64 instances of one size (1..3), limb count l and scale 2^a together.
 * Per coefficient the decrypted integer M in (-Q_l / 2, Q_l / 2] becomes M' = floor((M + 2^(t-1)) / 2^t) (t = 0: M), with
 * 2^t = scale / scale_out, 0 <= t <= 62: ties go towards +infinity.  M' is reduced under the first limbs_out chain
 * primes (limbs_out below, at or above l) and encrypted as evah_encode_encrypt_symmetric_sampled_many encrypts its
 * plaintexts: error drawn on the device from ekeys [n][32] (secret), c1 expanded from seeds [n][32] (public).
 * out: ONE batched handle [n][2][limbs_out][N] at scale_out, instances in list order, then instance order.  Exact integer
 * arithmetic throughout: every word follows from (cts, the secret key, limbs_out, t, ekeys, seeds).
 * Refusals: a capturing context, a limb shard, null pointers, "secret key not present", mismatches in the list by
 * argument index, more than 64 instances, a size outside 1..3, "invalid limb count for this context", a scale that is
 * not 2^a with a an integer, a target scale above the value's (t < 0), t > 62, N not divisible by 256.  One host -> device
 * copy of the keys (and one of the seeds above 8 instances), no device -> host copy, one drain of the queue;
 * evah_ctx_transfer_stats out[4] grows by 64 n.  The decrypted messages, the error keys and NTT(e) are zeroed on the
 * queue before their memory returns to the pool, also when the call fails. */
int evah_refresh_handles(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n_handles, uint32_t limbs_out, double scale_out,
                         const uint8_t *ekeys, const uint8_t *seeds, evah_ct **out);

/* ---- threshold decryption --------------------------------------------------------------------------
 * A result is opened by parties that each hold a share s_p of the secret key s = sum_p s_p, none of them the whole.
 * The two calls restate SEAL's Decryptor::decrypt (dot_product_ct_sk_array: c0 + c1 s) split over the parties, with the
 * noise flooding ("smudging") of the multiparty CKKS protocols in front of CKKSEncoder::decode; the reference
 * (seal.cpp:124-146, SEALSecret::decrypt) has the one-party form only.
 *
 * evah_decrypt_share_handles: on a context with the party's secret key s_p installed (evah_client_key_upload,
 * evah_keygen_*).  cts: what evah_decrypt_decode_handles takes, at most 64 instances of size 2, one limb count l and one
 * scale together, read in place.  Instance r gets h = c1 s_p + NTT(E) per limb (canonical residues), E drawn on the
 * device from fkeys[r] (32 bytes, SECRET: whoever learns E learns c1 s_p): coefficient j = word j % 8 of the ChaCha20
 * block j / 8 under the nonce 0x666c000000000000, E_j = (w >> (63 - smudge_bits)) - 2^smudge_bits, uniform on
 * [-2^smudge_bits, 2^smudge_bits).  out: ONE batched size-1 handle [n][1][l][N] at the ciphertexts' scale, instances in
 * list order, then instance order.  Refusals: a capturing context, a limb shard, "secret key not present", null
 * pointers, mismatches in the list by argument index, more than 64 instances, "decryption share expects a size-2
 * ciphertext (relinearize first)", smudge_bits outside 1..62, "smudge_bits leaves no room at this level"
 * (2^(smudge_bits + 2) > Q_l).  One host -> device copy of the keys, nothing back, one drain of the queue;
 * evah_ctx_transfer_stats out[4] grows by 32 n.  The keys are zeroed on the queue before their memory returns to the
 * pool, also when the call fails. */
int evah_decrypt_share_handles(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n_handles, uint32_t smudge_bits, const uint8_t *fkeys,
                               evah_ct **out);
/* evah_decrypt_combine_rows: m = c0 + sum_p h_p per limb, then everything evah_decrypt_decode_rows does behind its dot
 * product (inverse transforms, exact recomposition, the FFT, the gather into rows of dtype_out on the host or in device
 * memory, pitched; the same meaning of row_pitch, out_on_device and wait).  shares: n_parties (1..64) size-1 handles as
 * evah_decrypt_share_handles returns them, each holding the n instances of cts in the same order, with the ciphertexts'
 * limb count and scale; a share made elsewhere arrives through evah_ct_upload_batch.  Needs NO secret key: any context
 * over the same parameters can run it.  The caller refuses P 2^(smudge_bits + 2) > Q_l (a handle does not carry
 * smudge_bits); a slot then differs from the decryption under s by at most N P 2^smudge_bits / scale.  Refusals: a
 * capturing context, a limb shard, null pointers, mismatches by ciphertext or share index, more than 64 instances,
 * a size other than 2, and those of evah_decrypt_decode_rows for the rows. */
int evah_decrypt_combine_rows(evah_ctx *ctx, const evah_ct *const *cts, uint32_t n_handles, const evah_ct *const *shares, uint32_t n_parties,
                              uint32_t n_out, int dtype_out, void *out, size_t row_pitch, int out_on_device, int wait);

/* ---- whole-DAG submit: a topologically sorted flat op list over a value table.
 * One call replaces the per-node loop ProgramTraversal::forwardPass + SEALExecutor::operator()
 * (program_traversal.h:36-93, seal_executor.h:279-404) for the encrypted part of a program.
 *   op    : the reference's Op codes (eva/ir/ops.h:11-25): Negate 10, Add 11, Sub 12, Mul 13,
 *           RotateLeftConst 14, RotateRightConst 15, Relinearize 20, ModSwitch 21, Rescale 22,
 *           Output 2 (dst names the same ciphertext as src0); Input 1 / Constant 3 / Encode 23 are
 *           accepted as markers of caller-placed slots
 *   imm   : rotation steps (14/15), rescale divisor bits (22)
 *   flags : EVAH_OPF_FREE_SRC0/1 = the caller does not need that operand afterwards: it is released
 *           once its last reader in the list has run (the reference frees at last use under
 *           Galois, multicore_program_traversal.h:62-67).  The flags are optional and belong to the value,
 *           not to the reader: a slot is released iff SOME reader names it, and then after its LAST
 *           reader, whichever of them carried the flag — what running the list op by op and freeing
 *           the flagged operands once nobody reads them any more gives.  A slot nobody flags, and a
 *           dst nobody reads, stays with the caller; caller-placed slots may be flagged like any other.
 * Single assignment: every dst slot starts empty and is written by exactly one op; inputs and
 * encoded plaintexts (Encode / Constant nodes) are placed in the table by the caller; on return
 * the slots written by ops hold new handles owned by the caller (unless released by a flag).
 * Operand kinds select the evaluator call exactly as seal_executor.h:114-175 does: Add/Mul swap a
 * plaintext first operand behind the ciphertext, Mul with src0 == src1 is square, Sub needs a
 * ciphertext first (plain - cipher is "Unsupported operation encountered", as in evah_elementwise_program).
 * An op a single entry point would refuse fails the submit with that entry point's message; values the
 * caller did not flag are untouched by a failed submit.
 * Scheduling inside (same ciphertexts as running the list op by op): ops are taken level by level
 * (depth from the caller-placed values — what MulticoreProgramTraversal's ready set holds), the
 * independent rotations / rescales / relinearizations / ciphertext products of a level go out
 * through the batched entry points, a Relinearize read only by a Rescale is evaluated with it,
 * a Mul read only by such a Relinearize joins them (evah_multiply_relinearize_rescale_many),
 * multiply_plain / add chains without other readers become one evah_weighted_sum, and a Rotate whose
 * readers are all such products (the taps of a convolution window) is not evaluated on its own: the
 * sums that end at one level and share their rotations go out as one evah_rotate_weighted_sums.
 * r5: what is left of the elementwise ops (Negate / Add / Sub / Mul on intermediates: freeable, read by somebody,
 * every check of their entry point passing) is recorded, not run; when a rescale, key switch, rotation or output needs
 * one of them, every unevaluated op below it goes out as one evah_elementwise_program per (level, batch size), storing
 * only what an op outside the program reads (EVAH_EW_FUSE=0: one launch per op). */
enum { EVAH_VAL_NONE = 0, EVAH_VAL_CT = 1, EVAH_VAL_PT = 2 };
enum { EVAH_OPF_FREE_SRC0 = 1, EVAH_OPF_FREE_SRC1 = 2 };
typedef struct evah_val { uint32_t kind; void *h; } evah_val;
typedef struct evah_op { uint32_t op, dst, src0, src1; int32_t imm; uint32_t flags; } evah_op;
int evah_execute(evah_ctx *ctx, const evah_op *ops, uint32_t n_ops, evah_val *table, uint32_t n_vals);

/* ---- a straight-line program of elementwise evaluator calls in ONE launch (eva_amd/csrc/ewprogram.hip) ----------
 * Replaces a run of SEALExecutor's elementwise dispatches — add / sub (+ plain) seal_executor.h:114-150, multiply /
 * square / multiply_plain :152-175, negate :191-195 — on values nobody else reads: Harris' response
 * det - k trace^2 is seven such calls, Sobel's magnitude and polynomial a dozen (examples/image_processing.py:39-100).
 * Values 0 .. n_in-1 are the inputs (ciphertexts or plaintexts, as in evah_execute's table), value n_in + j is the
 * result of ops[j]; `op` is the Op code of /root/reference/eva/ir/ops.h:11-25 (10 Negate, 11 Add, 12 Sub, 13 Mul) with
 * SEALExecutor's dispatch rules: a plaintext first operand of Add / Mul goes behind the ciphertext, Mul(a, a) is
 * square, Sub keeps its order (plain - cipher is "Unsupported operation encountered", as in the reference).  Checks,
 * error messages and results are those of the separate entry points called in program order; intermediates that are not
 * listed in out_vals never reach HBM.  All ciphertexts of a program are of one level and batch size.  A program beyond
 * one launch's registers runs as the separate calls.  evah_execute builds these programs itself (EVAH_EW_FUSE). */
typedef struct evah_ew_op { uint32_t op, a, b; } evah_ew_op;
int evah_elementwise_program(evah_ctx *ctx, const evah_val *in, uint32_t n_in, const evah_ew_op *ops, uint32_t n_ops,
                             const uint32_t *out_vals, uint32_t n_out, evah_ct **outs);

/* ---- limb-sharded execution (BASELINE config 5) --------------------------
 * The RNS limbs of every value are dealt over G shards — limb i on shard i mod G — one shard per
 * GPU (one process per GPU, RCCL between them) or several shards in one process.  A shard is an
 * evah_ctx with a limb -> prime map: after evah_ctx_set_shard(ctx, s, G) the context's values hold
 * only the limbs s, s+G, ... (`limbs` of a handle is then the LOCAL count) and every per-limb entry
 * point above works on them unchanged; evah_mod_switch is called on the owner of the dropped limb
 * only.  The reference has no counterpart (its parallelism is node-level,
 * multicore_program_traversal.h:55-78): these entry points split the SEAL calls that mix limbs —
 * switch_key_inplace behind relinearize / rotate_vector (seal_executor.h:200, :181/:188) and
 * rescale_to_next (:213) — into phases with ONE exchange step between phases, done by the caller:
 *   key switch   ks_digits -> all-gather of the coefficient-form digits -> ks_products ->
 *                broadcast of r from the owner of the special limb (shard l mod G) -> ks_finish
 *   rescale      rescale_last on the owner of limb l-1 -> broadcast of r -> rescale_finish
 * `l` is the GLOBAL limb count of the level.  evah_buf is device memory for the exchange steps;
 * evah_buf_ptr exposes the device address (for torch / RCCL), evah_buf_copy is the in-process exchange. */
typedef struct evah_buf evah_buf;
int evah_ctx_set_shard(evah_ctx *ctx, uint32_t shard, uint32_t n_shards);
int evah_ctx_shard_info(evah_ctx *ctx, uint32_t *shard, uint32_t *n_shards);
int evah_buf_alloc(evah_ctx *ctx, size_t words, evah_buf **out);
void evah_buf_free(evah_ctx *ctx, evah_buf *buf);
/* zero the buffer on ctx's queue (the queue it was allocated from): what a holder of decrypted values does before
 * evah_buf_free returns the memory to the pool */
int evah_buf_wipe(evah_ctx *ctx, evah_buf *buf);
void *evah_buf_ptr(evah_buf *buf);
size_t evah_buf_words(const evah_buf *buf);
int evah_buf_copy(evah_ctx *dst_ctx, evah_buf *dst, size_t dst_off, const evah_buf *src, size_t src_off, size_t words);
/* one launch on dst's queue that pulls n (<= 64) chunks of `words` words: srcs[j][src_offs[j]..) -> dst[dst_offs[j]..)
 * (offsets and words even); sources on other devices are read as peers — the all-gather / broadcast of the phases above
 * as ONE kernel per receiving shard.  Stands where the reference's workers share memory
 * (multicore_program_traversal.h:55-78). */
int evah_buf_gather(evah_ctx *dst_ctx, evah_buf *dst, uint32_t n, const evah_buf *const *srcs, const size_t *src_offs,
                    const size_t *dst_offs, size_t words);
/* peer access between the devices of two contexts, both directions (hipDeviceCanAccessPeer + hipDeviceEnablePeerAccess);
 * a refusal is an error (evah_last_error names the pair), never a silent staging through the host.  Every multi-device
 * group calls it for each pair of its members before the first cross-device copy. */
int evah_ctx_enable_peer(evah_ctx *a, evah_ctx *b);
int evah_buf_download(evah_ctx *ctx, const evah_buf *buf, size_t off, size_t words, uint64_t *host);
int evah_buf_upload(evah_ctx *ctx, evah_buf *buf, size_t off, size_t words, const uint64_t *host);
/* (perm(c0), perm(c1)) on the local limbs: the NTT-domain Galois automorphism of rotate_vector */
int evah_shard_galois_perm(evah_ctx *ctx, const evah_ct *a, uint32_t galois_elt, evah_ct **out);
/* digits: [G][rows][N] words, rows >= ceil(l / G); row [s][j] = INTT of local limb j of polynomial `poly` */
int evah_shard_ks_digits(evah_ctx *ctx, const evah_ct *a, uint32_t poly, uint32_t l, evah_buf *digits, uint32_t rows);
/* prod: [2][ni][N] with ni = local data limbs (+1 on the owner of the special limb); r: [2][N] */
int evah_shard_ks_products(evah_ctx *ctx, const evah_ct *a, uint32_t poly, uint32_t l, const evah_buf *digits, uint32_t rows,
                           int key_kind, uint32_t galois_elt, evah_buf *prod, evah_buf *r);
/* out = (add's first add_polys polynomials, or nothing) + mod-down of prod, size 2, at `scale` */
int evah_shard_ks_finish(evah_ctx *ctx, uint32_t l, const evah_buf *prod, const evah_buf *r, const evah_ct *add,
                         uint32_t add_polys, double scale, evah_ct **out);
/* r: [size][N] */
int evah_shard_rescale_last(evah_ctx *ctx, const evah_ct *a, uint32_t l, evah_buf *r);
int evah_shard_rescale_finish(evah_ctx *ctx, const evah_ct *a, uint32_t l, const evah_buf *r, uint32_t divisor_bits,
                              evah_ct **out);

/* ---- whole-DAG capture ------------------------------------------------------------------------
 * Replaces the per-call DAG walk of SEALPublic::execute (seal.cpp:104-122) for repeated
 * executions of one compiled program: every evaluator call issued on `q0` and `others` (forks of
 * one context) between begin and end is recorded into a hipGraph, including the cross-queue
 * ordering; evah_graph_launch replays it on q0's stream.  Handles created before the capture
 * (inputs, pre-encoded plaintexts) and handles still alive at the end (outputs) keep their device
 * addresses; calls that synchronise with the host (uploads, downloads) are rejected while
 * capturing.  The temporaries of the captured walk are taken out of the queues' pools for the graph's
 * lifetime (every replay writes them again), so the queues stay usable for other work — e.g. copies of
 * the outputs enqueued on q0 right behind a replay — and evah_graph_free returns the blocks. */
int evah_capture_begin(evah_ctx *q0, evah_ctx **others, uint32_t n_others);
int evah_capture_end(evah_ctx *q0, evah_ctx **others, uint32_t n_others, evah_graph **out);
int evah_graph_launch(evah_ctx *q0, evah_graph *g);
void evah_graph_free(evah_graph *g);

/* ---- test / measurement hooks -------------------------------------------------------------- */
/* in-place negacyclic NTT (inverse=0) or INTT (inverse=1) of one host polynomial mod primes[i] */
int evah_test_ntt(evah_ctx *ctx, uint32_t prime_idx, int inverse, uint64_t *host_inout);
/* the device words of an installed relinearization / Galois key -> out: which = 0 the key as the kernels read it
 * ([n_digits][2][rows][N]; rows = k, or a limb shard's own rows), which = 1 its radix-2^30 split copy — an error when the
 * key has none (primes of another shape, EVAH_MAC3=0, a limb shard) */
int evah_test_key_words(evah_ctx *ctx, int kind, uint32_t galois_elt, int which, uint64_t *out);
/* One arithmetic primitive of the kernels (devmath.hip.h, the butterflies of ntt.hip.h, the key-switch accumulators of
 * ntt_ks_inner.hip.h) applied by a small kernel to n lanes of host words, with the DevPrime of primes[prime_idx].
 * Lane i reads a[i*m + j], b[i*m + j] for j < m (m > 1 only for the sequence ops ACC128, ACC128C, MAC3, KS128) and
 * c[2i], c[2i+1]; it writes out[2i], out[2i+1] (a single result in out[2i], a 128-bit one as (lo, hi), a butterfly as
 * (X, Y)).  Operands by op:
 *   MUL_SHOUP_LAZY, MUL_SHOUP, MUL_TW_LAZY5   x = a, w = b, w' = c[2i]
 *   MUL_TW_LAZY5_ADD(_MAD)                  the same, addend c[2i+1]
 *   BARRETT64 a;  BARRETT128, REDUCE128_LAZY  (lo, hi) = (a, b);  ADDMOD, SUBMOD a, b;  NEGMOD a;  TOPBIT a
 *   ACC128, ACC128C                         (c[2i], c[2i+1]) + sum_j a_j b_j
 *   MAC3                                    digits a_j, split key words b_j (k0 | k1 << 32); c[2i] != 0 overrides the
 *                                           fold period; refused unless the context's key switches may use MAC3
 *   KS128                                   lazy digits a_j, key words b_j, then three terms c[2i] c[2i+1]
 *   BFLY_FWD + (REDUCE | MAD << 1 | TB << 2), BFLY_INV   (X, Y) = (a, b), twiddle (w, w') = (c[2i], c[2i+1]) */
enum {
  EVAH_DM_MUL_SHOUP_LAZY = 0, EVAH_DM_MUL_SHOUP, EVAH_DM_BARRETT64, EVAH_DM_MUL_TW_LAZY5, EVAH_DM_MUL_TW_LAZY5_ADD,
  EVAH_DM_MUL_TW_LAZY5_ADD_MAD, EVAH_DM_BARRETT128, EVAH_DM_REDUCE128_LAZY, EVAH_DM_ACC128, EVAH_DM_ACC128C,
  EVAH_DM_ADDMOD, EVAH_DM_SUBMOD, EVAH_DM_NEGMOD, EVAH_DM_TOPBIT, EVAH_DM_MAC3, EVAH_DM_KS128, EVAH_DM_BFLY_INV,
  EVAH_DM_BFLY_FWD, EVAH_DM_COUNT = EVAH_DM_BFLY_FWD + 8
};
int evah_test_devmath(evah_ctx *ctx, uint32_t prime_idx, int op, uint32_t n, uint32_t m, const uint64_t *a,
                      const uint64_t *b, const uint64_t *c, uint64_t *out);
/* Per-launch HIP-event profile by kernel class (events are recorded on the launch stream around
 * every kernel launch while enabled); used by bench.py for the roofline of the dominant kernel. */
int evah_profile_enable(evah_ctx *ctx, int on);
int evah_profile_reset(evah_ctx *ctx);
int evah_profile_classes(void);
const char *evah_profile_class_name(int cls);
int evah_profile_get(evah_ctx *ctx, int cls, uint64_t *launches, double *total_ms);
/* HIP-event timing on the context's stream: start, stop -> elapsed milliseconds */
int evah_timer_start(evah_ctx *ctx);
int evah_timer_stop(evah_ctx *ctx, float *ms);

#ifdef __cplusplus
}
#endif
#endif
