// launch.hip.h — launch plumbing of the transform kernels (ntt.hip.h), shared by the translation
// units of libeva_hip.so that issue transforms: pass selection by size (8 / 4 coefficients per thread,
// the fused inverse + forward form for latency-bound launches), profiling classes, and the entry
// points of the key-switch core that keyswitch.hip defines for rotate.hip and shard.hip.
#pragma once
#include "internal.hip.h"
#include "ntt.hip.h"

namespace evah {

// 2 coefficients per thread (16-byte accesses); grid = (N/512, limbs, polys)
#define EW_SETUP                                                                                 \
  const uint32_t p = blockIdx.z, i = blockIdx.y;                                                 \
  const size_t off = (size_t)i * cx.N + 2 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x);    \
  const DevPrime pm = cx.primes[cx.prime_of(i)];                                                 \
  (void)p;                                                                                        \
  (void)pm;

__device__ __forceinline__ ulonglong2 ld2(const u64 *p) { return *reinterpret_cast<const ulonglong2 *>(p); }
__device__ __forceinline__ void st2(u64 *p, ulonglong2 v) { *reinterpret_cast<ulonglong2 *>(p) = v; }
// a key word cut at bit 30 (KeyDev::d_split): the operand form of the radix-2^30 inner product
__device__ __forceinline__ u64 split30(u64 k) { return (k & 0x3fffffffull) | ((k >> 30) << 32); }

// ---- NTT launch plumbing
template <class Op> struct OpClass;
template <bool Z, bool G> struct OpClass<OpPlainT<Z, G>> { static constexpr int fwd_a = KC_NTT_A, fwd_b = KC_NTT_B; };
template <> struct OpClass<OpMulIntt> { static constexpr int fwd_a = KC_NTT_A, fwd_b = KC_NTT_B; };
template <> struct OpClass<OpKsDigit> { static constexpr int fwd_a = KC_KSDIGIT_A, fwd_b = KC_KSDIGIT_B; };
template <bool G> struct OpClass<OpModDownT<G>> { static constexpr int fwd_a = KC_MODDOWN_A, fwd_b = KC_MODDOWN_B; };
template <> struct OpClass<OpMulPolyIntt> { static constexpr int fwd_a = KC_NTT_A, fwd_b = KC_NTT_B; };
template <> struct OpClass<OpModDownMul> { static constexpr int fwd_a = KC_MODDOWN_A, fwd_b = KC_MODDOWN_B; };
template <int M> struct OpClass<OpRRT<M>> { static constexpr int fwd_a = KC_MODDOWN_A, fwd_b = KC_MODDOWN_B; };
template <int M> struct OpClass<OpRRLastT<M>> { static constexpr int fwd_a = KC_MODDOWN_A, fwd_b = KC_MODDOWN_B; };
template <> struct OpClass<OpTailIntt> { static constexpr int fwd_a = KC_MODDOWN_A, fwd_b = KC_MODDOWN_B; };
template <> struct OpClass<OpChainIntt> { static constexpr int fwd_a = KC_NTT_A, fwd_b = KC_NTT_B; };
template <> struct OpClass<OpChainT> { static constexpr int fwd_a = KC_INTT_B, fwd_b = KC_INTT_B; };
template <> struct OpClass<OpChainDigit> { static constexpr int fwd_a = KC_KSDIGIT_A, fwd_b = KC_KSDIGIT_B; };
template <> struct OpClass<OpRsMd> { static constexpr int fwd_a = KC_MODDOWN_A, fwd_b = KC_MODDOWN_B; };

template <int P, int LR, bool STRIDED, bool INVERSE, class Op>
static void launch_pass(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  ProfScope ps(c, INVERSE ? (STRIDED ? KC_INTT_B : KC_INTT_A)
                          : (STRIDED ? OpClass<Op>::fwd_a : OpClass<Op>::fwd_b));
  const uint32_t max_tile = (uint32_t)NTT_THREADS << LR;
  const uint32_t tile = c->N < max_tile ? c->N : max_tile;
  const int logC = (int)ilog2(tile) - P;
  size_t lds = ((((size_t)1 << logC) * lds_sub_stride<P>() + 1) & ~(size_t)1) * sizeof(u64);
  if (STRIDED) lds += ((size_t)1 << P) * sizeof(ulonglong2); // staged twiddles
  lds += c->tun.lds_extra; // occupancy probe (EVAH_LDS_EXTRA), 0 ordinarily
  const uint32_t n_tiles = c->N / tile;
  const int log_tiles = (int)ilog2(n_tiles);
  dim3 grid = Op::grid(prm, jobs), block(tile >> LR);
  grid.x *= n_tiles;
  if (tile == max_tile) {
    hipLaunchKernelGGL((ntt_pass_kernel<P, LR, STRIDED, INVERSE, Op, true>), grid, block, lds, c->stream, c->dev,
                       prm, logC, log_tiles);
  } else if constexpr (P == 5) { // N = 1024: one partial tile per polynomial
    hipLaunchKernelGGL((ntt_pass_kernel<P, LR, STRIDED, INVERSE, Op, false>), grid, block, lds, c->stream, c->dev,
                       prm, logC, log_tiles);
  } else {
    throw std::logic_error("partial NTT tile with P != 5");
  }
  HIPCHK(hipGetLastError());
}

template <int LR, bool STRIDED, bool INVERSE, class Op>
static void launch_pass_lr(evah_ctx *c, int P, const typename Op::Params &prm, uint32_t jobs) {
  switch (P) {
  case 5: launch_pass<5, LR, STRIDED, INVERSE, Op>(c, prm, jobs); break;
  case 6: launch_pass<6, LR, STRIDED, INVERSE, Op>(c, prm, jobs); break;
  case 7: launch_pass<7, LR, STRIDED, INVERSE, Op>(c, prm, jobs); break;
  case 8: launch_pass<8, LR, STRIDED, INVERSE, Op>(c, prm, jobs); break;
  case 9:
    if constexpr (STRIDED) { launch_pass<9, LR, STRIDED, INVERSE, Op>(c, prm, jobs); break; }
    [[fallthrough]];
  default: throw std::runtime_error("unsupported poly_modulus_degree for the NTT kernels");
  }
}
// Contiguous pass as ntt_loop_kernel: one wave per 256-coefficient tile, the tile's twiddle heaps staged in LDS once
// and reused by up to loop_n jobs that share the prime (Tunables::loop_n; 0 = off).  Returns false when the launch
// has fewer than loop_min jobs along the op's loop axis (nothing to share) and the caller takes ntt_pass_kernel.
template <int P, bool INVERSE, class Op>
static bool launch_loop_pass(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  constexpr int LR = 2;
  dim3 grid = Op::grid(prm, jobs);
  uint32_t ext[3] = {grid.x, grid.y, grid.z};
  const uint32_t count = ext[Op::loop_axis];
  if (!c->tun.loop_n || count < c->tun.loop_min || c->N < 256) return false;
  // a launch that cannot fill the chip is latency-bound: walking jobs one after the other only lengthens it
  if ((uint64_t)ext[0] * ext[1] * ext[2] / count * (c->N / 256) * ((count + 1) / 2) < c->tun.loop_min_wgs) return false;
  ProfScope ps(c, INVERSE ? KC_INTT_A : OpClass<Op>::fwd_b);
  const uint32_t tile = 256, n_tiles = c->N / tile;
  const int logC = 8 - P, log_tiles = (int)ilog2(n_tiles);
  // enough workgroups to fill the chip several times over before twiddle sharing is taken further
  uint32_t nloop = std::min<uint32_t>(c->tun.loop_n, count);
  const uint64_t others = (uint64_t)ext[0] * ext[1] * ext[2] / count * n_tiles;
  while (nloop > 2 && others * ((count + nloop - 1) / nloop) < c->tun.loop_target_wgs) nloop = (nloop + 1) / 2;
  ext[Op::loop_axis] = (count + nloop - 1) / nloop;
  const size_t lds = ((((size_t)1 << logC) * lds_sub_stride<P>() + 1) & ~(size_t)1) * sizeof(u64) +
                     ((size_t)1 << (logC + P)) * sizeof(ulonglong2);
  hipLaunchKernelGGL((ntt_loop_kernel<P, LR, INVERSE, Op>), dim3(ext[0] * n_tiles, ext[1], ext[2]), dim3(tile >> LR), lds, c->stream,
                     c->dev, prm, logC, log_tiles, nloop, count);
  HIPCHK(hipGetLastError());
  // evah_ctx_loop_stats: which of its four profile classes the kernel ran as, its jobs and its walks along the loop axis
  constexpr int cls = INVERSE ? KC_INTT_A : OpClass<Op>::fwd_b;
  static_assert(cls == KC_INTT_A || cls == KC_NTT_B || cls == KC_KSDIGIT_B || cls == KC_MODDOWN_B, "a class evah_ctx_loop_stats has no word for");
  c->looped[cls == KC_INTT_A ? 0 : cls == KC_NTT_B ? 1 : cls == KC_KSDIGIT_B ? 2 : 3]++;
  c->looped[4] += count;
  c->looped[5] += ext[Op::loop_axis];
  return true;
}
template <bool INVERSE, class Op>
static bool launch_loop_pass_p(evah_ctx *c, int P, const typename Op::Params &prm, uint32_t jobs) {
  switch (P) {
  case 5: return launch_loop_pass<5, INVERSE, Op>(c, prm, jobs);
  case 6: return launch_loop_pass<6, INVERSE, Op>(c, prm, jobs);
  case 7: return launch_loop_pass<7, INVERSE, Op>(c, prm, jobs);
  case 8: return launch_loop_pass<8, INVERSE, Op>(c, prm, jobs);
  default: return false;
  }
}

// 8 coefficients per thread measured best for the stand-alone passes on MI355X (vs 4: +12 %,
// vs 16: +10 %, profiles/r01_tuning_notes.md); the fused key-switch kernel uses 4.
template <bool STRIDED, bool INVERSE, class Op>
static void launch_pass_p(evah_ctx *c, int P, const typename Op::Params &prm, uint32_t jobs) {
  if constexpr (!STRIDED) {
    if (launch_loop_pass_p<INVERSE, Op>(c, P, prm, jobs)) return;
  }
  // a launch that cannot fill the chip is bound by ONE wave's instruction stream (a thread's 8
  // coefficients are ~600 integer instructions per pass): with 4 coefficients per thread the same
  // tile work is spread over twice the workgroups and the critical path of a workgroup shrinks
  if (c->tun.small_lr == 2 && (uint64_t)jobs * (c->N >> 11) <= c->tun.small_lr_blocks && c->N >= 2048) {
    launch_pass_lr<2, STRIDED, INVERSE, Op>(c, P, prm, jobs);
    return;
  }
  launch_pass_lr<3, STRIDED, INVERSE, Op>(c, P, prm, jobs);
}

static_assert(WIDE_TILE == (uint32_t)NTT_THREADS << 3, "the mod-up, tail and small-launch kernels work on 8 coefficients per thread");

// what a batch of key switches reads beside the digits: the same in a caller's request (KsCall) and in a launch's header
struct KsOperands {
  size_t target_bs = 0;        // target of instance b = target + b * target_bs, or
  PtrTab targets{};            // targets.p[b] when the targets are separate allocations (target == nullptr)
  const MulTab *mul = nullptr; // fused multiply: the target of instance b is d2 = a1 b1 of product b
  bool fold = false;           // fused multiply: P * d0, P * d1 are added to the products here (KS_FOLDMUL; the target is then
                               // read from memory); without mul: P * adds.p[2b + K] is (KS_FOLDADD)
  const PtrTab *adds = nullptr;
  bool lazy_out = false;       // the data rows of prod may be any 64-bit representative (consumer: the relinearize + rescale combine)
};
struct KsBatch : KsOperands { // one launch worth of key-switches: regular strides, irregular keys
  uint32_t n = 1;
  uint32_t i0 = 0, ni = 0; // output-limb slice
  size_t scratch_bs = 0, prod_bs = 0;
  KsKeys keys{};
  bool mac3 = false;           // keys point at the split layout: ks_inner_kernel<MAC3> (radix-2^30 accumulation)
  uint32_t istep = 1, nout = 0; // output limbs I = i0 + y * istep; nout = rows per polynomial of prod (0: l + 1)
  u64 *r_out = nullptr; // != nullptr: the special row leaves as the first inverse pass of the mod-down (INVSP)
  bool diag = false;    // the diagonal digit comes from scratch too (no NTT-form target: the chain step, ntt_chain.hip.h)
  uint32_t fold_row = ~0u; // KS_FOLDMUL: != ~0u adds (P q_a^-1) d_K, a = fold_row, instead of P d_K
  // a slice of the relinearize + rescale key switch that runs the tail's contiguous passes itself (ks_inner_kernel TAIL;
  // prod is not written).  KS_TAIL_A: i0 = l - 1, ni = 2, r_out = r, tail_out.t = t; KS_TAIL_B: i0 = 0, ni = l - 1,
  // r_out = the output buffer, tail_out.dst_ps = its polynomial stride
  int tail = KS_TAIL_NONE;
  KsTailOut tail_out{};
};
// What relin_rescale_core hands switch_key_products when the key switch runs the tail's contiguous passes (TAIL_KS_SLICES):
// the launch set is mod-up, slice A, ntt_tail_kernel (lp, rp), slice B, and prod is never touched
struct KsTailPlan {
  OpRRLastFolded::Params lp; // r, t, last, sp (prod is not read)
  OpRRFolded::Params rp;     // dst = the output buffer, which slice B finishes in place (r, t, prod are not read)
};
// a caller's request to switch_key_products: n (target, key) pairs at one level
struct KsCall : KsOperands {
  const u64 *target = nullptr;         // targets at stride target_bs; nullptr: the table `targets`
  const KeyDev *const *keys = nullptr; // keys[b] switches instance b
  uint32_t n = 1;
  u64 *prod = nullptr;                 // [n][2][l + 1][N]; not written under a tail plan
  u64 *r = nullptr;                    // [2 n][N]: takes the special rows' first inverse pass where KsForm::special_inv
  const KsTailPlan *tail = nullptr;    // TAIL_KS_SLICES
};
// The operand table of pairs x B products of size-2 ciphertexts at level l — entry i * B + x is instance x of pair i —
// with the checks every call that multiplies makes of its operands (batch_msg: its text for a handle that does not hold
// B instances); the operands are acquired.  Returns the products' scales, one per pair.
inline std::vector<double> fill_mul_tab(evah_ctx *c, const evah_ct *const *as, const evah_ct *const *bs, uint32_t pairs, uint32_t B,
                                        uint32_t l, const char *batch_msg, MulTab &tab) {
  std::vector<double> scales(pairs);
  for (uint32_t i = 0; i < pairs; i++) {
    const evah_ct *a = as[i], *b = bs[i];
    if (a->size != 2 || b->size != 2) throw std::invalid_argument("multiply supports size-2 operands only (relinearize first)");
    if (a->batch != B || b->batch != B) throw std::invalid_argument(batch_msg);
    if (a->limbs != l || b->limbs != l) throw std::invalid_argument("encrypted parameter mismatch in batch");
    scales[i] = a->scale * b->scale;
    check_scale(c, scales[i], l);
    acquire(c, a->buf);
    acquire(c, b->buf);
    for (uint32_t x = 0; x < B; x++) {
      tab.a[i * B + x] = a->d + (size_t)x * 2 * a->ps;
      tab.b[i * B + x] = b->d + (size_t)x * 2 * b->ps;
      tab.a_ps[i * B + x] = (uint32_t)(a->ps / c->N);
      tab.b_ps[i * B + x] = (uint32_t)(b->ps / c->N);
    }
  }
  return scales;
}

// second (contiguous) pass of the digit transforms fused with the key inner product (keyswitch.hip)
void launch_ks_inner(evah_ctx *c, int P, const u64 *target, const u64 *scratch, const KsBatch &key, u64 *prod, uint32_t l);

template <class Op> static void ntt_forward(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  const int a = (c->logN + 1) / 2, b = c->logN / 2;
  launch_pass_p<true, false, Op>(c, a, prm, jobs);
  launch_pass_p<false, false, Op>(c, b, prm, jobs);
}
template <class Op> static void ntt_inverse(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  const int a = (c->logN + 1) / 2, b = c->logN / 2;
  launch_pass_p<false, true, Op>(c, b, prm, jobs);
  launch_pass_p<true, true, Op>(c, a, prm, jobs);
}

// ---- latency-bound launches: inverse strided pass + forward strided pass as one launch (ntt_inv_fwd_kernel)
static inline bool fuse_small_launch(evah_ctx *c, uint32_t fwd_jobs) {
  const uint32_t tile = (uint32_t)NTT_THREADS << 3;
  if (!c->tun.fuse_small_blocks || c->N < tile) return false; // partial tiles (N = 1024) keep the two-launch form
  if (c->dev.guard) return true; // a guarded (normally skipped) launch set: the fewest launches, whatever the size
  return (uint64_t)fwd_jobs * (c->N / tile) <= c->tun.fuse_small_blocks;
}

// ---- the launch form of a batch of n key switches at level l with keys[b]: chosen here, once per launch set, from ks_caps
// and the sizes; whoever launches takes it as given (DESIGN.md 4.6 lists form, condition and launches)
enum KsDigits { KS_DIGITS_SMALL, KS_DIGITS_MODUP, KS_DIGITS_SLICED, KS_DIGITS_UNFUSED }; // (the last: EVAH_FUSE_MAC=0)
// what follows the products: the mod-down, or one of the four relinearize + rescale tails
enum RelinTail { TAIL_MOD_DOWN, TAIL_KS_SLICES, TAIL_THREE, TAIL_FOLDED, TAIL_R03 };
struct KsForm {
  KsDigits digits;
  uint32_t groups;  // output-limb slices of KS_DIGITS_SLICED
  bool mac3;        // radix-2^30 accumulation: the context and the level admit it and every key has its split copy
  bool md_small;    // the mod-down that follows is a small launch
  bool special_inv; // the special rows' first inverse pass leaves the key-switch kernel in KsCall::r; prod's special rows are NOT written
  RelinTail tail;
};
// rescale: relinearize + rescale (a tail follows, not the mod-down); mul: the target is a product formed on load
static inline KsForm ks_form(evah_ctx *c, uint32_t l, const KeyDev *const *keys, uint32_t n, bool rescale = false, bool mul = false) {
  if (n < 1 || n > (uint32_t)KS_BATCH_MAX) throw std::runtime_error("key-switch batch out of range");
  const KsCaps k = ks_caps(c);
  KsForm f{};
  if (!c->tun.fuse_mac) f.digits = KS_DIGITS_UNFUSED;
  else if (k.groups == 1 && fuse_small_launch(c, n * (l + 1) * l)) f.digits = KS_DIGITS_SMALL;
  else f.digits = k.modup ? KS_DIGITS_MODUP : KS_DIGITS_SLICED;
  f.groups = std::min<uint32_t>(k.groups, l + 1);
  // (the r03 fused-multiply form, KS_MUL, has no radix-2^30 kernel)
  f.mac3 = k.mac3 && l <= MAC3_MAX_LIMBS && !(mul && !k.fold);
  for (uint32_t b = 0; b < n; b++) { // the keys: present for the level, whole, and in the split layout for mac3
    if (keys[b]->n_digits < l) throw std::runtime_error("key switching key has too few digits");
    if (keys[b]->rows != c->k) throw std::logic_error("this context holds a limb shard's key rows: use the evah_shard_* entry points");
    f.mac3 = f.mac3 && keys[b]->d_split;
  }
  // r5: the digit transforms may be throughput-sized while the mod-down that follows is still a small launch
  // (relinearize_many of Harris' three products: 3456 digit tiles, 768 mod-down tiles): the special rows' first inverse
  // pass then rides the key-switch kernel as it does in the small form (one launch of ~6 us less)
  f.md_small = !rescale && fuse_small_launch(c, 2 * n * l);
  f.special_inv = f.md_small && k.special_inv && f.digits != KS_DIGITS_UNFUSED && k.groups == 1;
  if (!rescale) f.tail = TAIL_MOD_DOWN;
  // slice A's 2 n N / 256 one-wave workgroups fill the chip (Tunables::ks_tail)
  else if (k.ks_tail_on && l >= 2 && f.digits == KS_DIGITS_MODUP && f.mac3 &&
           (uint64_t)2 * n * (c->N / (KS_WAVE << KS_LR)) >= k.ks_tail_min_wgs) f.tail = TAIL_KS_SLICES;
  else if (k.fold && k.tail3 && f.digits == KS_DIGITS_MODUP) f.tail = TAIL_THREE;
  else f.tail = k.fold ? TAIL_FOLDED : TAIL_R03;
  return f;
}
template <int P, class Op, int LR> static void launch_inv_fwd_plr(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  ProfScope ps(c, OpClass<Op>::fwd_a);
  const uint32_t tile = (uint32_t)NTT_THREADS << LR, n_tiles = c->N / tile;
  const int logC = (int)ilog2(tile) - P;
  const size_t lds = ((((size_t)1 << logC) * lds_sub_stride<P>() + 1) & ~(size_t)1) * sizeof(u64) + 2 * ((size_t)1 << P) * sizeof(ulonglong2);
  dim3 grid = Op::grid(prm, jobs);
  grid.x *= n_tiles;
  hipLaunchKernelGGL((ntt_inv_fwd_kernel<P, LR, Op>), grid, dim3(NTT_THREADS), lds, c->stream, c->dev, prm, (int)ilog2(n_tiles));
  HIPCHK(hipGetLastError());
}
template <int P, class Op> static void launch_inv_fwd_p(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  if (c->tun.small_lr == 2) launch_inv_fwd_plr<P, Op, 2>(c, prm, jobs);
  else launch_inv_fwd_plr<P, Op, 3>(c, prm, jobs);
}
template <class Op> static void launch_inv_fwd(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  switch ((c->logN + 1) / 2) {
  case 6: launch_inv_fwd_p<6, Op>(c, prm, jobs); break;
  case 7: launch_inv_fwd_p<7, Op>(c, prm, jobs); break;
  case 8: launch_inv_fwd_p<8, Op>(c, prm, jobs); break;
  case 9: launch_inv_fwd_p<9, Op>(c, prm, jobs); break;
  default: throw std::runtime_error("unsupported poly_modulus_degree for the fused inverse/forward pass");
  }
}
// ---- the key switch's mod-up at throughput size: strided inverse pass of each digit, then its conversion and forward
// strided pass under every output prime of prm (i0 = 0, istep = 1), one workgroup per (column tile, digit, instance) —
// ntt_modup_kernel (ntt_modup.hip.h).  n = instances; the digits' contiguous inverse pass left its intermediate in prm.t
// Both shapes (Tunables::modup_lr) work on 2048-coefficient tiles: KsCaps::wide_tile.
template <int P, int LR, class Op, bool TBONLY, bool LAZYONLY>
static void launch_modup_v(evah_ctx *c, const typename Op::Params &prm, uint32_t n) {
  ProfScope ps(c, OpClass<Op>::fwd_a);
  // 8 coefficients per thread: 256 threads; 4 per thread: 512 threads.  Either way a 2048-coefficient tile, 2^(11 - P)
  // columns wide — at P = 8 a row segment of 64 bytes (4 per thread on 256 threads, a 1024-coefficient tile with 32-byte
  // segments, ran 2.8 times slower: profiles/r08_modup_notes.md)
  constexpr int NT = LR == 2 ? 2 * NTT_THREADS : NTT_THREADS;
  const uint32_t tile = (uint32_t)NT << LR, n_tiles = c->N / tile;
  const int logC = (int)ilog2(tile) - P;
  const size_t lds = ((((size_t)1 << logC) * lds_sub_stride<P>() + 1) & ~(size_t)1) * sizeof(u64) + ((size_t)1 << P) * sizeof(ulonglong2);
  hipLaunchKernelGGL((ntt_modup_kernel<P, LR, Op, TBONLY, LAZYONLY, NT>), dim3(n_tiles * prm.l, 1, n), dim3(NT), lds, c->stream,
                     c->dev, prm, (int)ilog2(n_tiles));
  HIPCHK(hipGetLastError());
}
template <int P, class Op> static void launch_modup_p(evah_ctx *c, const typename Op::Params &prm, uint32_t n) {
  const ModupVariant v = modup_variant(c);
  auto go = [&](auto lrtag) {
    constexpr int LR = decltype(lrtag)::value;
    if (v.lazyonly) launch_modup_v<P, LR, Op, true, true>(c, prm, n);
    else if (v.tbonly) launch_modup_v<P, LR, Op, true, false>(c, prm, n);
    else launch_modup_v<P, LR, Op, false, false>(c, prm, n);
  };
  if (v.lr == 2) go(std::integral_constant<int, 2>{});
  else go(std::integral_constant<int, 3>{});
}
template <class Op> static void launch_modup(evah_ctx *c, const typename Op::Params &prm, uint32_t n) {
  if (!ks_caps(c).wide_tile || prm.i0 != 0 || prm.istep != 1) throw std::logic_error("mod-up kernel outside its shapes");
  switch ((c->logN + 1) / 2) {
  case 6: launch_modup_p<6, Op>(c, prm, n); break;
  case 7: launch_modup_p<7, Op>(c, prm, n); break;
  case 8: launch_modup_p<8, Op>(c, prm, n); break;
  case 9: launch_modup_p<9, Op>(c, prm, n); break;
  default: throw std::runtime_error("unsupported poly_modulus_degree for the mod-up kernel");
  }
}
// ---- the strided passes of the relinearize + rescale tail at throughput size, one workgroup per (column tile, polynomial):
// ntt_tail_kernel (ntt_tail.hip.h).  The contiguous inverse pass (OpTailIntt) left the special rows' intermediate in lp.r and
// the last rows' in lp.t; the lazy first-pass words of OpRRFolded go to rp.dst.  Same shapes as the mod-up (KsCaps::wide_tile).
template <int P, bool TBONLY, bool LAZYONLY>
static void launch_tail_v(evah_ctx *c, const OpRRLastFolded::Params &lp, const OpRRFolded::Params &rp, uint32_t polys) {
  ProfScope ps(c, KC_MODDOWN_A);
  const uint32_t tile = (uint32_t)NTT_THREADS << 3, n_tiles = c->N / tile;
  const int logC = (int)ilog2(tile) - P;
  const size_t lds = ((((size_t)1 << logC) * lds_sub_stride<P>() + 1) & ~(size_t)1) * sizeof(u64) + ((size_t)1 << P) * sizeof(ulonglong2);
  hipLaunchKernelGGL((ntt_tail_kernel<P, TBONLY, LAZYONLY>), dim3(n_tiles, 1, polys), dim3(NTT_THREADS), lds, c->stream, c->dev, lp, rp);
  HIPCHK(hipGetLastError());
}
// (a template so that only the translation unit that calls it instantiates the kernels)
template <class RR = OpRRFolded>
static void launch_tail(evah_ctx *c, const OpRRLastFolded::Params &lp, const typename RR::Params &rp, uint32_t polys) {
  if (!ks_caps(c).wide_tile || rp.jl < 1) throw std::logic_error("tail kernel outside its shapes");
  const TailVariant v = tail_variant(c);
  auto go = [&](auto ptag) {
    constexpr int P = decltype(ptag)::value;
    if (v.lazyonly) launch_tail_v<P, true, true>(c, lp, rp, polys);
    else if (v.tbonly) launch_tail_v<P, true, false>(c, lp, rp, polys);
    else launch_tail_v<P, false, false>(c, lp, rp, polys);
  };
  switch ((c->logN + 1) / 2) {
  case 6: go(std::integral_constant<int, 6>{}); break;
  case 7: go(std::integral_constant<int, 7>{}); break;
  case 8: go(std::integral_constant<int, 8>{}); break;
  case 9: go(std::integral_constant<int, 9>{}); break;
  default: throw std::runtime_error("unsupported poly_modulus_degree for the tail kernel");
  }
}
// two strided inverse passes + combine (+ strided forward pass): ntt_inv2_kernel (ntt_chain.hip.h)
template <int P, class Op, bool FWD, int LR> static void launch_inv2_plr(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  ProfScope ps(c, OpClass<Op>::fwd_a);
  const uint32_t tile = (uint32_t)NTT_THREADS << LR, n_tiles = c->N / tile;
  const int logC = (int)ilog2(tile) - P;
  const size_t lds = ((((size_t)1 << logC) * lds_sub_stride<P>() + 1) & ~(size_t)1) * sizeof(u64) + 2 * ((size_t)1 << P) * sizeof(ulonglong2);
  dim3 grid = Op::grid(prm, jobs);
  grid.x *= n_tiles;
  hipLaunchKernelGGL((ntt_inv2_kernel<P, LR, Op, FWD>), grid, dim3(NTT_THREADS), lds, c->stream, c->dev, prm, (int)ilog2(n_tiles));
  HIPCHK(hipGetLastError());
}
template <class Op, bool FWD> static void launch_inv2(evah_ctx *c, const typename Op::Params &prm, uint32_t jobs) {
  auto go = [&](auto ptag) {
    constexpr int P = decltype(ptag)::value;
    if (c->tun.small_lr == 2) launch_inv2_plr<P, Op, FWD, 2>(c, prm, jobs);
    else launch_inv2_plr<P, Op, FWD, 3>(c, prm, jobs);
  };
  switch ((c->logN + 1) / 2) {
  case 6: go(std::integral_constant<int, 6>{}); break;
  case 7: go(std::integral_constant<int, 7>{}); break;
  case 8: go(std::integral_constant<int, 8>{}); break;
  case 9: go(std::integral_constant<int, 9>{}); break;
  default: throw std::runtime_error("unsupported poly_modulus_degree for the fused inverse/forward pass");
  }
}
// inverse transform of the source limb(s) (InvOp jobs) followed by the forward transforms of Op:
// four launches, or three when the forward launch is too small to fill the chip
// inv_pass1_done: the contiguous inverse pass already left its intermediate in ip.dst (fused into the
// key-switch kernel); only ever set when fuse_small_launch(c, fwd_jobs) holds
template <class InvOp, class Op>
static void inverse_then_forward(evah_ctx *c, const typename InvOp::Params &ip, uint32_t inv_jobs, const typename Op::Params &fp,
                                 uint32_t fwd_jobs, bool inv_pass1_done = false) {
  if (inv_pass1_done && !fuse_small_launch(c, fwd_jobs)) throw std::logic_error("fused inverse pass outside the small-launch form");
  if (fuse_small_launch(c, fwd_jobs)) {
    if (!inv_pass1_done) launch_pass_p<false, true, InvOp>(c, c->logN / 2, ip, inv_jobs); // contiguous inverse pass: lazy intermediate in ip.dst
    launch_inv_fwd<Op>(c, fp, fwd_jobs);
    launch_pass_p<false, false, Op>(c, c->logN / 2, fp, fwd_jobs);
  } else {
    ntt_inverse<InvOp>(c, ip, inv_jobs);
    ntt_forward<Op>(c, fp, fwd_jobs);
  }
}

// ---- defined in keyswitch.hip
// steps 1-2 of SEAL's switch_key_inplace for a batch of n (target, key) pairs in the form f (see the definition)
void switch_key_products(evah_ctx *c, uint32_t l, const KsCall &q, const KsForm &f);

// ---- key switch + mod-down (steps 1-3)
// the special rows of prod[polys][l + 1][N] through the inverse transform into r[polys][N], + P/2: what every mod-down starts with
inline OpPlain::Params special_rows_intt(const evah_ctx *c, uint32_t l, const u64 *prod, u64 *r) {
  return OpPlain::Params{prod + (size_t)l * c->N, r, (size_t)(l + 1) * c->N, c->N, 1, c->k - 1, 1, {}};
}
// the caller's side of a mod-down's combine pass: add[K] (stride add_ps; K < add_polys, ~0u: even polys only) joins, the result
// goes to dst; add_tab / use_add_tab or add_bs are set on the result where they apply
inline OpModDown::Params md_combine(const u64 *add, size_t add_ps, uint32_t add_polys, u64 *dst, size_t dst_ps) {
  return OpModDown::Params{nullptr, 0, nullptr, 0, add, add_ps, add_polys, dst, dst_ps, 0, 0};
}
// step 3 for the products of n key switches in the form f: INTT(special rows) + P/2, then per-limb NTT + combine (mp: md_combine).
// f.special_inv: switch_key_products left the first inverse pass in r and did not write the special rows.
// (templates so that only the translation units that call them instantiate the kernels)
template <class MD = OpModDown>
static void ks_mod_down(evah_ctx *c, uint32_t l, uint32_t n, const KsForm &f, const u64 *prod, u64 *r, typename MD::Params mp) {
  mp.r = r, mp.r_ps = c->N;
  mp.c = prod, mp.c_ps = (size_t)(l + 1) * c->N;
  mp.a = c->k - 1, mp.jl = l;
  inverse_then_forward<OpPlain, MD>(c, special_rows_intt(c, l, prod, r), 2 * n, mp, 2 * n * l, f.special_inv);
}
// steps 1-3: out[b][K] = (the combine side of mp) + keyswitch(target_b)[K]; q.prod and q.r are supplied here
template <class MD = OpModDown>
static void switch_key_mod_down(evah_ctx *c, uint32_t l, KsCall q, const typename MD::Params &mp) {
  Scratch prod(c, (size_t)q.n * 2 * (l + 1) * c->N), r(c, (size_t)q.n * 2 * c->N);
  const KsForm f = ks_form(c, l, q.keys, q.n);
  q.prod = prod.d, q.r = r.d;
  switch_key_products(c, l, q, f);
  ks_mod_down<MD>(c, l, q.n, f, prod.d, r.d, mp);
}
void switch_key(evah_ctx *c, uint32_t l, const u64 *target, const KeyDev &key, const u64 *add, size_t add_ps, uint32_t add_polys,
                u64 *out, size_t out_ps);
// ---- defined in elementwise.hip: dst[i] = (src[i] mod 2^30) | (src[i] >> 30) << 32 (KeyDev::d_split)
void key_split_launch(evah_ctx *c, const u64 *src, u64 *dst, size_t words);
// ---- defined in rotate.hip: NTT-domain permutation table of a Galois element, cached per device state
const uint32_t *perm_table(evah_ctx *c, uint32_t elt);
// out[p][i][n] = a[p][i][perm[n]] for p < polys over `limbs` limbs (the NTT-domain Galois automorphism)
void galois_perm_launch(evah_ctx *c, const u64 *a, size_t a_ps, uint32_t limbs, uint32_t polys, const uint32_t *perm, u64 *out, size_t o_ps);
// ---- defined in elementwise.hip: FP64 root / slot tables of the CKKS encoder, built on first use
void enc_tables(evah_ctx *c);

} // namespace evah
