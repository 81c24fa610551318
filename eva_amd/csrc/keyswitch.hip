// keyswitch.hip — libeva_hip.so: the key-switch core (SEAL Evaluator::switch_key_inplace, SURVEY.md A.6: digit decomposition, the fused
// second pass + key inner product, mod-down) and the evaluator calls built on it or on the same transforms:
// relinearize, rescale_to_next and their fused / batched forms (/root/reference/eva/seal/seal_executor.h:197-215).
#include "launch.hip.h"

namespace evah {

// K9 inner product: prod[K][I] = sum_J op(I,J) * key[J][K][kappa(I)],
// op(I,J) = target[J] when I == J, else scratch[I][J].  128-bit lazy accumulation, one Barrett
// reduction at the end.  grid = (N/512, l+1).
__global__ void __launch_bounds__(256)
k_ks_mac(DevCtx cx, const u64 *target, const u64 *scratch, const u64 *key, u64 *prod, uint32_t l) {
  if (cx.skipped()) return;
  const uint32_t I = blockIdx.y;
  const uint32_t kap = (I == l) ? cx.k - 1 : I;
  const size_t n = 2 * ((size_t)blockIdx.x * blockDim.x + threadIdx.x);
  const DevPrime pm = cx.primes[kap];
  const size_t N = cx.N, key_digit = (size_t)2 * cx.k * N;
  u128_t a0x = {0, 0}, a0y = {0, 0}, a1x = {0, 0}, a1y = {0, 0};
  for (uint32_t J = 0; J < l; J++) {
    const u64 *op = (I == J) ? target + (size_t)J * N : scratch + ((size_t)I * l + J) * N;
    const ulonglong2 o = ld2(op + n);
    const u64 *kp = key + J * key_digit + (size_t)kap * N + n;
    const ulonglong2 k0 = ld2(kp), k1 = ld2(kp + (size_t)cx.k * N);
    acc128(a0x, o.x, k0.x);
    acc128(a0y, o.y, k0.y);
    acc128(a1x, o.x, k1.x);
    acc128(a1y, o.y, k1.y);
  }
  ulonglong2 r0, r1;
  r0.x = barrett128(a0x, pm);
  r0.y = barrett128(a0y, pm);
  r1.x = barrett128(a1x, pm);
  r1.y = barrett128(a1y, pm);
  st2(prod + (size_t)I * N + n, r0);
  st2(prod + ((size_t)(l + 1) + I) * N + n, r1);
}

// the header of a launch set of n key switches at level l in the form f, instance b with keys[b] (ks_form saw them): strides
// of the converted digits and of prod, the key pointers — the split copies under f.mac3
static KsBatch ks_batch(evah_ctx *c, uint32_t l, const KeyDev *const *keys, uint32_t n, const KsForm &f) {
  KsBatch kb;
  kb.n = n, kb.mac3 = f.mac3;
  kb.scratch_bs = (size_t)(l + 1) * l * c->N, kb.prod_bs = (size_t)2 * (l + 1) * c->N;
  for (uint32_t b = 0; b < n; b++) kb.keys.key[b] = kb.mac3 ? keys[b]->d_split : keys[b]->d;
  return kb;
}

template <int P>
static void launch_ks_inner_p(evah_ctx *c, const u64 *target, const u64 *scratch, const KsBatch &kb, u64 *prod, uint32_t l) {
  constexpr int LR = KS_LR;
  ProfScope ps(c, KC_KSMAC);
  const KsCaps caps = ks_caps(c);
  const uint32_t tile = caps.wg_threads << LR;
  const bool one_wave = caps.one_wave;
  const int logC = (int)ilog2(tile) - P;
  if (logC < 0) throw std::runtime_error("ks_inner tile smaller than one sub-transform");
  // coefficients tile + per-sub twiddle heaps (16 B per node)
  const size_t lds = ((((size_t)1 << logC) * lds_sub_stride<P>() + 1) & ~(size_t)1) * sizeof(u64) +
                     ((size_t)1 << (logC + P)) * sizeof(ulonglong2) +
                     (kb.mac3 ? (size_t)tile * sizeof(u64) : 0); // MAC3: the unpadded tile the LDS-DMA loads fill
  const uint32_t n_tiles = c->N / tile;
  // the one-wave workgroup (the default) is compiled with its own launch bound: the register
  // allocator is not held to the 256-thread budget
  auto go_tail = [&](auto kernel, const auto &mt, const auto &at, const auto &tl) {
    hipLaunchKernelGGL(kernel, dim3(n_tiles * kb.n, kb.ni), dim3(tile >> LR), lds, c->stream, c->dev, target, kb.target_bs, scratch,
                       kb.scratch_bs, kb.keys, prod, kb.prod_bs, l, kb.i0, logC, n_tiles, kb.n, kb.targets, mt, kb.istep,
                       kb.nout ? kb.nout : l + 1, kb.r_out, at, (kb.lazy_out ? 1 : 0) | (kb.diag ? 2 : 0), kb.fold_row, tl);
  };
  auto go = [&](auto kernel, const auto &mt, const auto &at) { go_tail(kernel, mt, at, NoMul{}); };
  if (kb.r_out && !kb.tail && (!one_wave || kb.istep != 1)) throw std::logic_error("fused special-row inverse pass needs the one-wave key-switch kernel");
  if (kb.fold && kb.istep != 1) throw std::logic_error("the folded key-switch forms are not used on limb shards");
  if (kb.fold && !kb.mul && !kb.adds) throw std::logic_error("folded key switch without polynomials to fold");
  if (kb.tail) {
    // the slices' rows are fixed: the kernel tells the special row from the last one, and a data row from both, by them
    const bool rows_ok = kb.tail == KS_TAIL_A ? (kb.i0 + 1 == l && kb.ni == 2 && kb.tail_out.t) : (kb.i0 == 0 && kb.ni + 1 == l && kb.tail_out.dst_ps);
    if (P < 6 || !kb.mac3 || !one_wave || !kb.fold || kb.istep != 1 || kb.diag || kb.fold_row != ~0u || !kb.r_out || l < 2 || !rows_ok)
      throw std::logic_error("key-switch tail epilogue outside its form");
  }
  const int mode = kb.mul ? (kb.fold ? KS_FOLDMUL : KS_MUL) : (kb.fold ? KS_FOLDADD : KS_PLAIN);
  auto with_mode = [&](auto mode_tag) {
    constexpr int M = decltype(mode_tag)::value;
    const KsMulArg<M> mt = [&] { if constexpr (M == KS_MUL || M == KS_FOLDMUL) return *kb.mul; else return NoMul{}; }();
    const KsAddArg<M> at = [&] { if constexpr (M == KS_FOLDADD) return *kb.adds; else return NoMul{}; }();
    if constexpr ((M == KS_FOLDMUL || M == KS_FOLDADD) && P >= 6) { // (the mod-up these slices follow needs N >= 2048)
      if (kb.tail == KS_TAIL_A) { go_tail(ks_inner_kernel<P, LR, 64, M, false, true, KS_TAIL_A>, mt, at, kb.tail_out); return; }
      if (kb.tail == KS_TAIL_B) { go_tail(ks_inner_kernel<P, LR, 64, M, false, true, KS_TAIL_B>, mt, at, kb.tail_out); return; }
    }
    if constexpr (M != KS_MUL) { // radix-2^30 accumulation: the one-wave kernels of the current forms
      if (kb.mac3 && one_wave) {
        if (kb.r_out) go(ks_inner_kernel<P, LR, 64, M, true, true>, mt, at);
        else go(ks_inner_kernel<P, LR, 64, M, false, true>, mt, at);
        return;
      }
    }
    if (kb.mac3) throw std::logic_error("split keys handed to a key-switch kernel that accumulates in 128 bits");
    if (kb.r_out) go(ks_inner_kernel<P, LR, 64, M, true>, mt, at);
    else if (one_wave) go(ks_inner_kernel<P, LR, 64, M>, mt, at);
    else go(ks_inner_kernel<P, LR, NTT_THREADS, M>, mt, at);
  };
  switch (mode) {
  case KS_PLAIN: with_mode(std::integral_constant<int, KS_PLAIN>{}); break;
  case KS_MUL: with_mode(std::integral_constant<int, KS_MUL>{}); break;
  case KS_FOLDMUL: with_mode(std::integral_constant<int, KS_FOLDMUL>{}); break;
  default: with_mode(std::integral_constant<int, KS_FOLDADD>{}); break;
  }
  HIPCHK(hipGetLastError());
}
void launch_ks_inner(evah_ctx *c, int P, const u64 *target, const u64 *scratch, const KsBatch &key, u64 *prod, uint32_t l) {
  switch (P) {
  case 5: launch_ks_inner_p<5>(c, target, scratch, key, prod, l); break;
  case 6: launch_ks_inner_p<6>(c, target, scratch, key, prod, l); break;
  case 7: launch_ks_inner_p<7>(c, target, scratch, key, prod, l); break;
  case 8: launch_ks_inner_p<8>(c, target, scratch, key, prod, l); break;
  default: throw std::runtime_error("unsupported poly_modulus_degree for the key-switch kernel");
  }
}

// SEAL Evaluator::switch_key_inplace, device version.
//   out[K] = (add && K < add_polys ? add[K] : 0) + keyswitch(target)[K],  K in {0,1}
// steps 1-2 of switch_key for a batch of q.n (target, key) pairs in one set of launches, in the form f = ks_form(...) of
// the caller: prod[b][K][I] (I <= l, slot l = special prime) = sum_J op_b(I,J) * key_b[J][K].
// target_b = q.target + b * q.target_bs (or q.targets.p[b]); prod_b = q.prod + b * 2 (l+1) N.
// f.special_inv: the special rows' first inverse pass leaves in q.r[2 n][N] and the special rows of prod are NOT written.
void switch_key_products(evah_ctx *c, uint32_t l, const KsCall &q, const KsForm &f) {
  const size_t N = c->N;
  const uint32_t n = q.n;
  const MulTab *const mul = q.mul;
  const bool fold = q.fold;
  KsBatch kb = ks_batch(c, l, q.keys, n, f);
  static_cast<KsOperands &>(kb) = q;
  if ((mul || fold) && !c->tun.fuse_mac) throw std::logic_error("the fused multiply / folded forms need the fused key-switch kernel");
  if ((q.tail ? f.tail != TAIL_KS_SLICES : f.tail == TAIL_KS_SLICES || !q.prod) || (f.special_inv && !q.r))
    throw std::logic_error("key-switch request lacks what its form writes");
  Scratch t(c, (size_t)n * l * N);        // coefficient-form digits
  Scratch sc(c, n * kb.scratch_bs);       // converted digits, NTT form per output limb
  // folded fused multiply: d2 is stored by the inverse transform that forms it and is the target from memory
  Scratch d2(c, mul && fold ? (size_t)n * l * N : 1);
  const u64 *target = q.target;
  if (mul && fold) {
    target = d2.d;
    kb.target_bs = (size_t)l * N;
  }
  // 1. digits to coefficient form (job -> (b, J))
  OpKsDigit::Params dp{t.d, sc.d, l, (size_t)l * N, kb.scratch_bs, 0, l + 1};
  // KS_DIGITS_SMALL: the digits' strided inverse pass and the first pass of the digit conversion run as one launch;
  // KS_DIGITS_MODUP: the strided inverse pass of each digit tile runs once, in the workgroup that converts it for every
  // output prime — either way t is the contiguous pass's intermediate, never the canonical digits
  const bool pass1_only = f.digits == KS_DIGITS_SMALL || f.digits == KS_DIGITS_MODUP;
  if (mul) { // the target is the product's d2, formed on load
    OpMulIntt::Params ip{*mul, t.d, (size_t)l * N, l, fold ? d2.d : nullptr};
    if (pass1_only) launch_pass_p<false, true, OpMulIntt>(c, c->logN / 2, ip, n * l);
    else ntt_inverse<OpMulIntt>(c, ip, n * l);
  } else {
    OpPlain::Params ip{target, t.d, kb.target_bs, (size_t)l * N, l, 0, 0, q.targets};
    if (pass1_only) launch_pass_p<false, true, OpPlain>(c, c->logN / 2, ip, n * l);
    else ntt_inverse<OpPlain>(c, ip, n * l);
  }
  if (f.special_inv) kb.r_out = q.r;
  if (f.digits == KS_DIGITS_SMALL) {
    dp.i0 = kb.i0 = 0;
    dp.ni = kb.ni = l + 1;
    launch_inv_fwd<OpKsDigit>(c, dp, n * (l + 1) * l);
    launch_ks_inner(c, c->logN / 2, target, sc.d, kb, q.prod, l);
    return;
  }
  if (f.digits != KS_DIGITS_UNFUSED) { // 128-bit accumulation of lazy (<16q) products, folded every 16 digits
    // Output limbs are processed in slices so that a slice's converted digits (ni * l * N words)
    // are still in L2 / Infinity Cache when the fused second pass consumes them.
    const int a = (c->logN + 1) / 2, b = c->logN / 2;
    if (const KsTailPlan *tail = q.tail) { // (the mod-up in one slice: ks_form)
      dp.i0 = 0;
      dp.ni = l + 1;
      launch_modup<OpKsDigit>(c, dp, n);
      // slice A: the last and the special rows, leaving as the contiguous inverse pass's intermediates in t and r
      kb.tail = KS_TAIL_A;
      kb.i0 = l - 1;
      kb.ni = 2;
      kb.r_out = const_cast<u64 *>(tail->lp.r);
      kb.tail_out = KsTailOut{tail->lp.t, 0};
      launch_ks_inner(c, b, target, sc.d, kb, nullptr, l);
      // both strided inverse passes and the correction's strided forward pass under every output prime, first-pass words
      // to the output buffer
      launch_tail(c, tail->lp, tail->rp, 2 * n);
      // slice B: the data rows below the last, each workgroup finishing the output words of its tile in place
      kb.tail = KS_TAIL_B;
      kb.i0 = 0;
      kb.ni = l - 1;
      kb.r_out = tail->rp.dst;
      kb.tail_out = KsTailOut{nullptr, tail->rp.dst_ps};
      launch_ks_inner(c, b, target, sc.d, kb, nullptr, l);
      return;
    }
    for (uint32_t g = 0; g < f.groups; g++) {
      const uint32_t i0 = (uint32_t)((uint64_t)(l + 1) * g / f.groups), i1 = (uint32_t)((uint64_t)(l + 1) * (g + 1) / f.groups);
      if (i1 == i0) continue;
      dp.i0 = kb.i0 = i0;
      dp.ni = kb.ni = i1 - i0;
      // 2a. base-convert + first (strided) NTT pass of every digit under the slice's output primes (the mod-up: with the
      // digits' strided inverse pass in front, all output primes in one slice)
      if (f.digits == KS_DIGITS_MODUP) launch_modup<OpKsDigit>(c, dp, n);
      else launch_pass_p<true, false, OpKsDigit>(c, a, dp, n * (i1 - i0) * l);
      // 2b. second (contiguous) pass fused with the inner product with the key
      launch_ks_inner(c, b, target, sc.d, kb, q.prod, l);
    }
  } else {
    // unfused reference path (EVAH_FUSE_MAC=0): full digit NTTs, then a separate MAC kernel
    ntt_forward<OpKsDigit>(c, dp, n * (l + 1) * l);
    for (uint32_t b = 0; b < n; b++) {
      ProfScope ps(c, KC_KSMAC);
      hipLaunchKernelGGL(k_ks_mac, dim3(c->N / 512, l + 1), dim3(256), 0, c->stream, c->dev,
                         target ? target + b * kb.target_bs : q.targets.p[b], sc.d + b * kb.scratch_bs, q.keys[b]->d,
                         q.prod + b * kb.prod_bs, l);
      HIPCHK(hipGetLastError());
    }
  }
}

void switch_key(evah_ctx *c, uint32_t l, const u64 *target, const KeyDev &key, const u64 *add,
                       size_t add_ps, uint32_t add_polys, u64 *out, size_t out_ps) {
  const KeyDev *kp = &key;
  KsCall q;
  q.target = target, q.keys = &kp;
  // fold_pa: P * add[K] goes into the inner products (KS_FOLDADD), the combine pass then adds nothing
  q.fold = ks_caps(c).fold && add && add_polys >= 1 && add_polys <= 2;
  PtrTab adds{};
  for (uint32_t K = 0; K < add_polys && q.fold; K++) adds.p[K] = add + K * add_ps;
  q.adds = q.fold ? &adds : nullptr;
  switch_key_mod_down(c, l, q, md_combine(q.fold ? nullptr : add, add_ps, add_polys, out, out_ps));
}

// ---- the size-3 entry points: checks, instance tables, one body per operation
// What every entry point that relinearizes asks of its n handles: the key, size 3, one level (at least 2 where a rescale
// follows: rescales) and B instances per handle (batch_msg: the entry point's text for a handle that holds another
// number).  The handles are acquired.
static void check_size3(evah_ctx *c, const evah_ct *const *as, uint32_t n, uint32_t B, bool rescales, const char *batch_msg) {
  if (!c->sh->relin.d) throw std::invalid_argument("relinearization key not present");
  for (uint32_t i = 0; i < n; i++) {
    const evah_ct *a = as[i];
    if (rescales && a->limbs < 2) throw std::invalid_argument("end of modulus switching chain reached");
    if (a->size != 3) throw std::invalid_argument("relinearize expects a size-3 ciphertext");
    if (a->batch != B) throw std::invalid_argument(batch_msg);
    if (a->limbs != as[0]->limbs) throw std::invalid_argument("encrypted parameter mismatch in batch");
    acquire(c, a->buf);
  }
}
// n (<= KS_BATCH_MAX) size-3 ciphertexts by address: c2.p[i] is the key-switch target of instance i, c01.p[2 i + K] the
// polynomial its result K is added to
struct Size3Tab {
  PtrTab c2{}, c01{};
  void set(uint32_t i, const u64 *d, size_t ps) {
    c2.p[i] = d + 2 * ps;
    c01.p[2 * i] = d;
    c01.p[2 * i + 1] = d + ps;
  }
};
// the instances of one handle through body(n, table of the n instances, first instance), KS_BATCH_MAX at a time
template <class Body> static void size3_chunks(const evah_ct *a, Body body) {
  for (uint32_t b0 = 0; b0 < a->batch; b0 += KS_BATCH_MAX) {
    const uint32_t n = std::min<uint32_t>(KS_BATCH_MAX, a->batch - b0);
    Size3Tab tab;
    for (uint32_t b = 0; b < n; b++) tab.set(b, a->d + (size_t)(b0 + b) * 3 * a->ps, a->ps);
    body(n, tab, b0);
  }
}

// relinearize: n (<= KS_BATCH_MAX) size-3 ciphertexts of l limbs in one launch set -> out_d[n][2][l N]
static void relin_core(evah_ctx *c, uint32_t l, uint32_t n, const Size3Tab &in, u64 *out_d) {
  std::vector<const KeyDev *> keys(n, &c->sh->relin);
  KsCall q;
  q.targets = in.c2, q.keys = keys.data(), q.n = n;
  // fold_pa: P * c_K goes into the inner products (KS_FOLDADD), the combine pass then adds nothing
  q.fold = ks_caps(c).fold;
  q.adds = q.fold ? &in.c01 : nullptr;
  OpModDown::Params mp = md_combine(nullptr, 0, 0, out_d, (size_t)l * c->N);
  mp.use_add_tab = !q.fold;
  mp.add_tab = in.c01;
  switch_key_mod_down(c, l, q, mp);
}

// relinearize + rescale_to_next: n (<= KS_BATCH_MAX) size-3 ciphertexts of l limbs -> out_d[n][2][(l-1) N], one set of
// n-times-wider launches; instances are co-scheduled per XCD so the key tiles are read from HBM once per XCD, not once
// per instance.
// mul != nullptr: instance b is the product a[b] x b[b] of mul (size-2 operands of l limbs), its polynomials d0, d1, d2
// evaluated where they are consumed (in == nullptr then)
static void relin_rescale_core(evah_ctx *c, uint32_t l, uint32_t n, const Size3Tab *in, const MulTab *mul, u64 *out_d) {
  const uint32_t last = l - 1, sp = c->k - 1;
  const size_t N = c->N, pps = (size_t)(l + 1) * N, ops = (size_t)(l - 1) * N;
  PtrTab c2{}, a_last{}, a_polys{};
  if (in) {
    c2 = in->c2;
    a_polys = in->c01;
    for (uint32_t i = 0; i < 2 * n; i++) a_last.p[i] = a_polys.p[i] + (size_t)last * N;
  }
  std::vector<const KeyDev *> keys(n, &c->sh->relin);
  const KsForm f = ks_form(c, l, keys.data(), n, /*rescale=*/true, mul != nullptr);
  KsCall q;
  q.targets = c2, q.keys = keys.data(), q.n = n, q.mul = mul;
  // r04: P * (the polynomials the key-switch result is added to) goes into the inner products themselves, so the
  // combine passes below read prod only (Tunables::fold_pa; the r03 forms stay for A/B runs, and for EVAH_FUSE_MAC=0)
  const bool fold = q.fold = f.tail != TAIL_R03;
  q.adds = mul ? nullptr : &a_polys;
  q.lazy_out = fold;
  // the folded tail's two ops on prod (null: the key-switch slices, which never store it), r and t
  auto folded = [&](const u64 *prod_d, u64 *r_d, u64 *t_d) {
    return KsTailPlan{OpRRLastFolded::Params{nullptr, 0, prod_d ? prod_d + (size_t)last * N : nullptr, pps, r_d, N, t_d, N, last, sp, {}},
                      OpRRFolded::Params{r_d, N, t_d, N, nullptr, 0, prod_d, pps, out_d, ops, sp, last, l - 1, {}}};
  };
  if (f.tail == TAIL_KS_SLICES) {
    // r10: five launches — the key-switch kernel runs the tail's two contiguous passes on the tiles it holds, as two
    // row slices around ntt_tail_kernel; prod is not allocated (KsCaps::ks_tail_on: which contexts, and why)
    Scratch r(c, (size_t)n * 2 * N), t(c, (size_t)n * 2 * N);
    const KsTailPlan plan = folded(nullptr, r.d, t.d);
    q.tail = &plan;
    switch_key_products(c, l, q, f);
    return;
  }
  Scratch prod(c, (size_t)n * 2 * pps);
  q.prod = prod.d;
  switch_key_products(c, l, q, f);
  Scratch r(c, (size_t)n * 2 * N), t(c, (size_t)n * 2 * N);
  const KsTailPlan p = folded(prod.d, r.d, t.d);
  if (f.tail == TAIL_THREE) {
    // the tail in three launches where the key switch above took the mod-up kernel (the RR_MEM / RR_MUL forms keep the
    // six below): contiguous inverse pass of the special and the last rows together; both strided inverse passes, r_K
    // and t_K in registers, and OpRRFolded's strided pass under every output prime (ntt_tail_kernel); its contiguous pass
    OpTailIntt::Params ip{p.lp, prod.d + (size_t)l * N, pps, r.d};
    launch_pass_p<false, true, OpTailIntt>(c, c->logN / 2, ip, 4 * n);
    launch_tail(c, p.lp, p.rp, 2 * n);
    launch_pass_p<false, false, OpRRFolded>(c, c->logN / 2, p.rp, 2 * n * (l - 1));
    return;
  }
  // r_K = INTT_P(prod[K][special]) + P/2
  ntt_inverse<OpPlain>(c, special_rows_intt(c, l, prod.d, r.d), 2 * n);
  if (fold) { // prod already carries P a[K]
    ntt_inverse<OpRRLastFolded>(c, p.lp, 2 * n);
    ntt_forward<OpRRFolded>(c, p.rp, 2 * n * (l - 1));
  } else if (mul) {
    OpRRLastMul::Params lp{nullptr, 0, prod.d + (size_t)last * N, pps, r.d, N, t.d, N, last, sp, a_last, *mul};
    ntt_inverse<OpRRLastMul>(c, lp, 2 * n);
    OpRRMul::Params rp{r.d, N, t.d, N, nullptr, 0, prod.d, pps, out_d, ops, sp, last, l - 1, a_polys, *mul};
    ntt_forward<OpRRMul>(c, rp, 2 * n * (l - 1));
  } else {
    // t_K = INTT_last(a[K][last] + prod[K][last] P^-1) - u_K,last P^-1 + q_last/2
    OpRRLast::Params lp{nullptr, 0, prod.d + (size_t)last * N, pps, r.d, N, t.d, N, last, sp, a_last};
    ntt_inverse<OpRRLast>(c, lp, 2 * n);
    // out[K][i] = (a[K][i] + prod[K][i] P^-1 - NTT_i(u P^-1 + v)) q_last^-1
    OpRR::Params rp{r.d, N, t.d, N, nullptr, 0, prod.d, pps, out_d, ops, sp, last, l - 1, a_polys};
    ntt_forward<OpRR>(c, rp, 2 * n * (l - 1));
  }
}

static double pow2(uint32_t bits) { return std::pow(2.0, (double)bits); }

// multiply (size 2 x size 2) -> relinearize -> rescale_to_next for n (<= 64) independent pairs at one
// level, the three SEAL calls of seal_executor.h:164, :200, :213-214 evaluated together: the size-3
// product is never materialised — d2 = a1 b1 is formed in the load of the digit inverse
// transform (and in the key-switch kernel where the NTT-form digit is used as is), d0 and d1 in
// the epilogue that combines them with the key-switch result.  Same ciphertext, bit for bit.
static void mul_relin_rescale(evah_ctx *c, const evah_ct *const *as, const evah_ct *const *bs, uint32_t n, uint32_t divisor_bits,
                              evah_ct **outs) {
  if (!c->tun.fuse_mac) { // the unfused reference path has no kernel that forms d2 on the fly: the three calls in turn
    std::vector<evah_ct *> prods(n, nullptr);
    if (evah_multiply_many(c, as, bs, n, prods.data())) throw std::runtime_error(g_err);
    const int rc = evah_relinearize_rescale_many(c, prods.data(), n, divisor_bits, outs);
    const std::string msg = g_err;
    for (evah_ct *p : prods) evah_ct_free(c, p);
    if (rc) throw std::runtime_error(msg);
    return;
  }
  if (n < 1 || n > (uint32_t)KS_BATCH_MAX) throw std::invalid_argument("multiply_relinearize_rescale_many handles 1..64 products per call");
  if (!c->sh->relin.d) throw std::invalid_argument("relinearization key not present");
  const uint32_t l = as[0]->limbs;
  if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
  MulTab tab{};
  const std::vector<double> scales = fill_mul_tab(c, as, bs, n, 1, l, "multiply_relinearize_rescale_many takes single ciphertexts", tab);
  FreshBuf ob(c, (size_t)n * 2 * (l - 1) * c->N);
  relin_rescale_core(c, l, n, nullptr, &tab, ob.d());
  ct_views(c, ob, n, 2, l - 1, 1, [&](uint32_t i) { return scales[i] / pow2(divisor_bits); }, outs);
}

// multiply (size 2 x size 2; a == b: square) -> rescale_to_next -> relinearize for n (<= 64) independent pairs at one level:
// the order lazy relinearization gives a product under the waterline rescalers (seal_executor.h:164 / :162, :213-214, :200).
// The size-3 product is never written — its polynomials are formed where the rescale reads them (OpMulPolyIntt,
// OpModDownMul).  Same ciphertext, bit for bit, as the three calls.
// The chain step in six launches (ntt_chain.hip.h: the rescaled d2 formed in coefficient form where the digit decomposition
// wants it; the rescale of d0 / d1 and the mod-down sharing one forward transform through (P L^-1) d_K folded into the inner
// products).  For ordinary contexts with whole keys and full transform tiles; anything else keeps the forms below.
static bool chain_step_applies(evah_ctx *c) {
  const KsCaps k = ks_caps(c);
  return c->tun.chain_step && k.fold && k.groups == 1 && c->dev.pstep == 1 && c->dev.p0 == 0 && !c->dev.guard && c->N >= WIDE_TILE &&
         c->sh->relin.rows == c->k;
}
// stored: instance b is a STORED size-3 ciphertext at tab.a[b] (polynomial stride tab.a_ps[b], tab.b[b] == nullptr) instead of
// the product tab.a[b] x tab.b[b] — Rescale -> Relinearize of a sum of products (evah_rescale_relinearize)
static void chain_step(evah_ctx *c, const MulTab &tab, uint32_t n, uint32_t l, u64 *out_d, bool stored = false) {
  const uint32_t lp = l - 1, last = l - 1, sp = c->k - 1;
  const size_t N = c->N, ops = (size_t)lp * N, pps = (size_t)(lp + 1) * N;
  const std::vector<const KeyDev *> keys(n, &c->sh->relin);
  const KsForm f = ks_form(c, lp, keys.data(), n); // (of its fields the chain step takes mac3, md_small and special_inv)
  KsBatch kb = ks_batch(c, lp, keys.data(), n, f);
  Scratch t2(c, (size_t)n * l * N), r01(c, (size_t)n * 2 * N);
  // 1. products + contiguous inverse pass: every limb of d2, limb L of d0 and d1
  OpChainIntt::Params ip{tab, t2.d, r01.d, l};
  launch_pass_p<false, true, OpChainIntt>(c, c->logN / 2, ip, n * (l + 2));
  // 2. t_J = rescaled d2 in coefficient form, digit conversion, strided forward pass
  PtrTab adds{};
  if (stored) { // (P L^-1) c_K from memory: KS_FOLDADD
    for (uint32_t b = 0; b < n; b++)
      for (uint32_t K = 0; K < 2; K++) adds.p[2 * b + K] = tab.a[b] + (size_t)K * tab.a_ps[b] * N;
    kb.adds = &adds;
  } else {
    kb.mul = &tab;
  }
  kb.fold = true;
  kb.fold_row = last;
  kb.diag = true;
  kb.i0 = 0;
  kb.ni = lp + 1;
  Scratch sc(c, n * kb.scratch_bs);
  const uint32_t dig_jobs = n * (lp + 1) * lp;
  if (fuse_small_launch(c, dig_jobs) && (uint64_t)dig_jobs * (c->N >> 11) <= c->tun.chain_fuse_blocks) {
    OpChainDigit::Params dp{t2.d, sc.d, l, kb.scratch_bs};
    launch_inv2<OpChainDigit, true>(c, dp, dig_jobs);
  } else {
    Scratch t(c, (size_t)n * lp * N);
    OpChainT::Params tp{t2.d, t.d, l};
    launch_inv2<OpChainT, false>(c, tp, n * lp);
    OpKsDigit::Params dp{t.d, sc.d, lp, (size_t)lp * N, kb.scratch_bs, 0, lp + 1};
    dp.diag = true;
    launch_pass_p<true, false, OpKsDigit>(c, (c->logN + 1) / 2, dp, dig_jobs);
    // (t is released in stream order: the digit pass above is enqueued before anything that could reuse it)
  }
  // 3. contiguous forward pass + key inner product + (P L^-1) d_K; the special limb's contiguous inverse pass when the
  //    mod-down is a small launch
  Scratch prod(c, (size_t)n * 2 * pps), r(c, (size_t)n * 2 * N);
  if (f.special_inv) kb.r_out = r.d;
  launch_ks_inner(c, c->logN / 2, nullptr, sc.d, kb, prod.d, lp);
  // 4. / 5. one forward transform per (K, i) for the rescale of d_K and the mod-down of prod_K
  OpRsMd::Params fp{r01.d, r.d, out_d, ops, last, sp, lp};
  OpModDown::Params mp{r.d, N, prod.d, pps, nullptr, 0, 0, out_d, ops, sp, lp};
  const OpPlain::Params spp = special_rows_intt(c, lp, prod.d, r.d);
  if (f.md_small) {
    if (!f.special_inv) launch_pass_p<false, true, OpPlain>(c, c->logN / 2, spp, 2 * n);
    launch_inv2<OpRsMd, true>(c, fp, 2 * n * lp);
  } else {
    ntt_inverse<OpPlain>(c, spp, 2 * n);
    OpPlain::Params lpp{r01.d, r01.d, N, N, 1, last, 1, {}}; // second (strided) pass of limb L of d0 / d1, in place
    launch_pass_p<true, true, OpPlain>(c, (c->logN + 1) / 2, lpp, 2 * n);
    launch_pass_p<true, false, OpRsMd>(c, (c->logN + 1) / 2, fp, 2 * n * lp);
  }
  launch_pass_p<false, false, OpModDown>(c, c->logN / 2, mp, 2 * n * lp);
}

static void mul_rescale_relin(evah_ctx *c, const evah_ct *const *as, const evah_ct *const *bs, uint32_t pairs, uint32_t divisor_bits, evah_ct **outs) {
  // batched handles (r6): every operand holds B instances; product i of instance b is entry i * B + b of the launch set, so the
  // outputs of one pair are contiguous — a batched handle again.  pairs * B <= 64 per call.
  const uint32_t B = pairs ? as[0]->batch : 0;
  if (pairs < 1 || B < 1 || (uint64_t)pairs * B > (uint64_t)KS_BATCH_MAX)
    throw std::invalid_argument("multiply_rescale_relinearize_many handles 1..64 products per call (pairs x instances of a batched handle)");
  const uint32_t n = pairs * B;
  if (!c->sh->relin.d) throw std::invalid_argument("relinearization key not present");
  const uint32_t l = as[0]->limbs;
  if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
  const uint32_t lp = l - 1, last = l - 1;
  const size_t N = c->N, ops = (size_t)lp * N, pps = (size_t)(lp + 1) * N;
  MulTab tab{};
  const std::vector<double> scales = fill_mul_tab(c, as, bs, pairs, B, l, "multiply_rescale_relinearize_many: operands of one call hold the same number of instances", tab);
  FreshBuf ob(c, (size_t)n * 2 * ops);
  if (chain_step_applies(c)) {
    chain_step(c, tab, n, l, ob.d());
  } else if (!c->tun.side_stream) {
    // one stream (the default: inside a replayed hipGraph a fork / join costs more than the overlap returns — config 5
    // 1.56 ms either way, r06_tuning_notes.md): the rescale of the three polynomials as one launch set, then the
    // relinearize of the stored result
    Scratch dp(c, (size_t)n * 3 * ops), r3(c, (size_t)n * 3 * N);
    OpMulPolyIntt::Params ip{tab, r3.d, 0, 3, last, 1};
    OpModDownMul::Params mpr{r3.d, tab, dp.d, ops, 0, 3, last, lp};
    inverse_then_forward<OpMulPolyIntt, OpModDownMul>(c, ip, 3 * n, mpr, 3 * n * lp);
    Size3Tab in;
    for (uint32_t b = 0; b < n; b++) in.set(b, dp.d + (size_t)3 * b * ops, ops);
    relin_core(c, lp, n, in, ob.d());
  } else {
    // two streams (EVAH_SIDE_STREAM=1; pays on eager walks: config 5 1.77 -> 1.70 ms): the rescale of d2 followed by its
    // key switch on the queue's stream, the rescale of d0 and d1 beside them on the queue's side stream; the halves meet in
    // the mod-down's combine, which adds d0' and d1'
    Scratch dp2(c, (size_t)n * ops), dp01(c, (size_t)n * 2 * ops), r3(c, (size_t)n * 3 * N);
    u64 *r01 = r3.d, *r2 = r3.d + (size_t)2 * n * N;
    SideStream side(c);
    // d2' = rescale(d2): what the key switch starts from
    OpMulPolyIntt::Params ip2{tab, r2, 2, 1, last, 1};
    OpModDownMul::Params mp2{r2, tab, dp2.d, ops, 2, 1, last, lp};
    inverse_then_forward<OpMulPolyIntt, OpModDownMul>(c, ip2, n, mp2, n * lp);
    // d0', d1' beside it
    side.fork();
    OpMulPolyIntt::Params ip01{tab, r01, 0, 2, last, 1};
    OpModDownMul::Params mp01{r01, tab, dp01.d, ops, 0, 2, last, lp};
    inverse_then_forward<OpMulPolyIntt, OpModDownMul>(c, ip01, 2 * n, mp01, 2 * n * lp);
    side.back();
    // key switch of d2' (the products only; d0', d1' join in the combine)
    Scratch prod(c, (size_t)n * 2 * pps), r(c, (size_t)n * 2 * N);
    std::vector<const KeyDev *> keys(n, &c->sh->relin);
    const KsForm f = ks_form(c, lp, keys.data(), n);
    KsCall q;
    q.target = dp2.d, q.target_bs = ops, q.keys = keys.data(), q.n = n;
    q.prod = prod.d, q.r = r.d;
    switch_key_products(c, lp, q, f);
    side.join();
    OpModDown::Params mp = md_combine(dp01.d, ops, 2, ob.d(), ops);
    mp.add_bs = 2 * ops;
    ks_mod_down(c, lp, n, f, prod.d, r.d, mp);
  }
  ct_views(c, ob, pairs, 2, lp, B, [&](uint32_t i) { return scales[i] / pow2(divisor_bits); }, outs);
}

// rescale_to_next of a size-3 ciphertext followed by relinearize (seal_executor.h:213-214, :200) — what lazy relinearization
// leaves after a SUM of products (Sobel's Ix^2 + Iy^2, Harris' response) — as the chain step on stored polynomials: n handles
// of B instances each, n * B <= 64.  Same ciphertext as the two calls.
static void rescale_relin(evah_ctx *c, const evah_ct *const *as, uint32_t pairs, uint32_t divisor_bits, evah_ct **outs) {
  const uint32_t B = pairs ? as[0]->batch : 0;
  if (pairs < 1 || B < 1 || (uint64_t)pairs * B > (uint64_t)KS_BATCH_MAX)
    throw std::invalid_argument("rescale_relinearize_many handles 1..64 ciphertexts per call (handles x instances of a batched handle)");
  check_size3(c, as, pairs, B, /*rescales=*/true, "rescale_relinearize_many: the handles of one call hold the same number of instances");
  const uint32_t l = as[0]->limbs, n = pairs * B;
  if (!chain_step_applies(c)) { // the two calls
    for (uint32_t i = 0; i < pairs; i++) {
      evah_ct *r = nullptr;
      int rc = evah_rescale(c, as[i], divisor_bits, &r);
      if (!rc) rc = evah_relinearize(c, r, &outs[i]);
      const std::string msg = g_err;
      if (r) evah_ct_free(c, r);
      if (rc) { // nothing of a failed call stays behind
        for (uint32_t j = 0; j < i; j++) {
          evah_ct_free(c, outs[j]);
          outs[j] = nullptr;
        }
        throw std::runtime_error(msg);
      }
    }
    return;
  }
  MulTab tab{};
  for (uint32_t i = 0; i < pairs; i++)
    for (uint32_t x = 0; x < B; x++) {
      tab.a[i * B + x] = as[i]->d + (size_t)x * 3 * as[i]->ps;
      tab.a_ps[i * B + x] = (uint32_t)(as[i]->ps / c->N);
    }
  FreshBuf ob(c, (size_t)n * 2 * (l - 1) * c->N);
  chain_step(c, tab, n, l, ob.d(), /*stored=*/true);
  ct_views(c, ob, pairs, 2, l - 1, B, [&](uint32_t i) { return as[i]->scale / pow2(divisor_bits); }, outs);
}

} // namespace evah

extern "C" {

// a batched handle: all instances in one launch set (chunks of KS_BATCH_MAX)
int evah_relinearize(evah_ctx *c, const evah_ct *a, evah_ct **out) {
  API_BEGIN
  use(c);
  check_size3(c, &a, 1, a->batch, /*rescales=*/false, "");
  const uint32_t l = a->limbs;
  FreshBuf ob(c, (size_t)a->batch * 2 * l * c->N);
  size3_chunks(a, [&](uint32_t n, const Size3Tab &in, uint32_t b0) { relin_core(c, l, n, in, ob.d() + (size_t)b0 * 2 * l * c->N); });
  ct_views(c, ob, 1, 2, l, a->batch, [&](uint32_t) { return a->scale; }, out);
  API_END
}

int evah_relinearize_rescale(evah_ctx *c, const evah_ct *a, uint32_t divisor_bits, evah_ct **out) {
  API_BEGIN
  use(c);
  check_size3(c, &a, 1, a->batch, /*rescales=*/true, "");
  const uint32_t l = a->limbs;
  FreshBuf ob(c, (size_t)a->batch * 2 * (l - 1) * c->N);
  size3_chunks(a, [&](uint32_t n, const Size3Tab &in, uint32_t b0) {
    relin_rescale_core(c, l, n, &in, nullptr, ob.d() + (size_t)b0 * 2 * (l - 1) * c->N);
  });
  ct_views(c, ob, 1, 2, l - 1, a->batch, [&](uint32_t) { return a->scale / pow2(divisor_bits); }, out);
  API_END
}

// n (<= 64) independent size-3 ciphertexts at the same level, all relinearized with the (shared) relinearization key and
// rescaled, as one launch set
int evah_relinearize_rescale_many(evah_ctx *c, const evah_ct *const *as, uint32_t n, uint32_t divisor_bits, evah_ct **outs) {
  API_BEGIN
  use(c);
  if (n < 1 || n > (uint32_t)KS_BATCH_MAX) throw std::invalid_argument("relinearize_rescale_many handles 1..64 ciphertexts per call");
  check_size3(c, as, n, 1, /*rescales=*/true, "relinearize_rescale_many takes single ciphertexts (a batched handle goes through evah_relinearize_rescale)");
  const uint32_t l = as[0]->limbs;
  Size3Tab in;
  for (uint32_t b = 0; b < n; b++) in.set(b, as[b]->d, as[b]->ps);
  FreshBuf ob(c, (size_t)n * 2 * (l - 1) * c->N);
  relin_rescale_core(c, l, n, &in, nullptr, ob.d());
  ct_views(c, ob, n, 2, l - 1, 1, [&](uint32_t b) { return as[b]->scale / pow2(divisor_bits); }, outs);
  API_END
}

int evah_multiply_relinearize_rescale_many(evah_ctx *c, const evah_ct *const *as, const evah_ct *const *bs, uint32_t n,
                                           uint32_t divisor_bits, evah_ct **outs) {
  API_BEGIN
  use(c);
  mul_relin_rescale(c, as, bs, n, divisor_bits, outs);
  API_END
}

int evah_multiply_relinearize_rescale(evah_ctx *c, const evah_ct *a, const evah_ct *b, uint32_t divisor_bits, evah_ct **out) {
  API_BEGIN
  use(c);
  if (a->batch != 1 || b->batch != 1 || !c->tun.fuse_mac) { // batched handles, the unfused path: the separate (already batched) calls
    evah_ct *m = nullptr;
    if (evah_multiply(c, a, b, &m)) throw std::runtime_error(g_err);
    int rc = evah_relinearize_rescale(c, m, divisor_bits, out);
    std::string err = g_err;
    evah_ct_free(c, m);
    if (rc) throw std::runtime_error(err);
  } else {
    mul_relin_rescale(c, &a, &b, 1, divisor_bits, out);
  }
  API_END
}

int evah_multiply_rescale_relinearize_many(evah_ctx *c, const evah_ct *const *as, const evah_ct *const *bs, uint32_t n, uint32_t divisor_bits,
                                           evah_ct **outs) {
  API_BEGIN
  use(c);
  mul_rescale_relin(c, as, bs, n, divisor_bits, outs);
  API_END
}
int evah_multiply_rescale_relinearize(evah_ctx *c, const evah_ct *a, const evah_ct *b, uint32_t divisor_bits, evah_ct **out) {
  API_BEGIN
  use(c);
  mul_rescale_relin(c, &a, &b, 1, divisor_bits, out);
  API_END
}

int evah_rescale_relinearize_many(evah_ctx *c, const evah_ct *const *as, uint32_t n, uint32_t divisor_bits, evah_ct **outs) {
  API_BEGIN
  use(c);
  rescale_relin(c, as, n, divisor_bits, outs);
  API_END
}
int evah_rescale_relinearize(evah_ctx *c, const evah_ct *a, uint32_t divisor_bits, evah_ct **out) {
  API_BEGIN
  use(c);
  rescale_relin(c, &a, 1, divisor_bits, out);
  API_END
}

// n independent ciphertexts of one size and level rescaled in one launch set (n * size <= 128)
int evah_rescale_many(evah_ctx *c, const evah_ct *const *cts, uint32_t n, uint32_t divisor_bits, evah_ct **outs) {
  API_BEGIN
  use(c);
  const uint32_t size = cts[0]->size, l = cts[0]->limbs;
  if (n < 1 || (size_t)n * size > 2 * KS_BATCH_MAX) throw std::invalid_argument("rescale_many: too many polynomials for one call");
  if (l < 2) throw std::invalid_argument("end of modulus switching chain reached");
  const size_t N = c->N, ops = (size_t)(l - 1) * N;
  const uint32_t polys = n * size;
  PtrTab last{}, all{};
  for (uint32_t b = 0; b < n; b++) {
    const evah_ct *a = cts[b];
    if (a->size != size || a->limbs != l) throw std::invalid_argument("encrypted parameter mismatch in batch");
    if (a->batch != 1) throw std::invalid_argument("rescale_many takes single ciphertexts");
    acquire(c, a->buf);
    for (uint32_t p = 0; p < size; p++) {
      all.p[b * size + p] = a->d + (size_t)p * a->ps;
      last.p[b * size + p] = a->d + (size_t)p * a->ps + (size_t)(l - 1) * N;
    }
  }
  FreshBuf ob(c, (size_t)polys * ops);
  Scratch r(c, (size_t)polys * N);
  OpPlain::Params ip{nullptr, r.d, 0, N, 1, l - 1, 1, last};
  OpModDown::Params mp{r.d, N, nullptr, 0, nullptr, 0, 0, ob.d(), ops, l - 1, l - 1};
  mp.c_tab = all;
  inverse_then_forward<OpPlain, OpModDown>(c, ip, polys, mp, polys * (l - 1));
  ct_views(c, ob, n, size, l - 1, 1, [&](uint32_t b) { return cts[b]->scale / pow2(divisor_bits); }, outs);
  API_END
}

// n (<= 64) independent size-3 ciphertexts of one level relinearized in one launch set
int evah_relinearize_many(evah_ctx *c, const evah_ct *const *cts, uint32_t n, evah_ct **outs) {
  API_BEGIN
  use(c);
  if (n < 1 || n > (uint32_t)KS_BATCH_MAX) throw std::invalid_argument("relinearize_many handles 1..64 ciphertexts per call");
  check_size3(c, cts, n, 1, /*rescales=*/false, "relinearize_many takes single ciphertexts");
  const uint32_t l = cts[0]->limbs;
  Size3Tab in;
  for (uint32_t b = 0; b < n; b++) in.set(b, cts[b]->d, cts[b]->ps);
  FreshBuf ob(c, (size_t)n * 2 * l * c->N);
  relin_core(c, l, n, in, ob.d());
  ct_views(c, ob, n, 2, l, 1, [&](uint32_t b) { return cts[b]->scale; }, outs);
  API_END
}

// Re-key: every instance of the handles through the key switch with the re-key key of `slot`, c1 the
// target and c0 the polynomial added to K = 0 — evah_rotate's call without the permutation.  The instances are read where
// they are, through the pointer tables (handles of another device state on this GPU behind acquire()), KS_BATCH_MAX per
// launch set; the results share one buffer, handle i viewing as many instances as cts[i] holds.
int evah_rekey_many(evah_ctx *c, uint32_t slot, const evah_ct *const *cts, uint32_t n_handles, evah_ct **outs) {
  API_BEGIN
  use(c);
  if (c->capturing) throw std::logic_error("re-key cannot be captured into a graph");
  if (c->dev.pstep > 1) throw std::invalid_argument("re-key is not available on a limb shard");
  if (!cts || !outs) throw std::invalid_argument("ciphertext list pointer is null");
  if (n_handles < 1) throw std::invalid_argument("re-key needs at least one ciphertext");
  auto kit = c->sh->rekey.find(slot);
  if (kit == c->sh->rekey.end()) throw std::invalid_argument("re-key key not present");
  const KeyDev *key = &kit->second;
  size_t total = 0;
  for (uint32_t i = 0; i < n_handles; i++) {
    const evah_ct *a = cts[i];
    if (!a) throw std::invalid_argument("ciphertext pointer is null");
    if (a->size != 2) throw std::invalid_argument("re-key expects a size-2 ciphertext (relinearize first)");
    if (a->limbs != cts[0]->limbs) throw std::invalid_argument("encrypted parameter mismatch in batch");
    const evah_ctx *owner = a->buf->owner;
    if (owner != c && ctx_alive(owner)) { // a value of another context: the same GPU and the same parameters
      if (owner->device != c->device) throw std::invalid_argument("the ciphertext lives on another GPU (copy it first: evah_ct_copy)");
      if (owner->N != c->N || owner->primes != c->primes) throw std::invalid_argument("the ciphertext's parameters differ from this context's");
    }
    total += a->batch;
  }
  const uint32_t l = cts[0]->limbs;
  if (l < 1 || l > c->k - 1) throw std::invalid_argument("invalid limb count for this context");
  for (uint32_t i = 0; i < n_handles; i++) acquire(c, cts[i]->buf);
  const size_t pps = (size_t)l * c->N;
  FreshBuf ob(c, total * 2 * pps);
  // (handle, instance) pairs in list order, a chunk at a time
  uint32_t h = 0, b = 0;
  for (size_t i0 = 0; i0 < total; i0 += KS_BATCH_MAX) {
    const uint32_t n = (uint32_t)std::min<size_t>(KS_BATCH_MAX, total - i0);
    PtrTab c1{}, c0{};
    for (uint32_t x = 0; x < n; x++) {
      const evah_ct *a = cts[h];
      const u64 *inst = a->d + (size_t)b * 2 * a->ps;
      c0.p[2 * x] = inst; // nothing is added to K = 1
      c1.p[x] = inst + a->ps;
      if (++b == a->batch) b = 0, h++;
    }
    std::vector<const KeyDev *> keys(n, key);
    KsCall q;
    q.targets = c1, q.keys = keys.data(), q.n = n;
    q.fold = ks_caps(c).fold; // P * c0 joins the inner product of K = 0 (KS_FOLDADD); otherwise the combine pass adds c0
    q.adds = q.fold ? &c0 : nullptr;
    OpModDown::Params mp = md_combine(nullptr, 0, 0, ob.d() + i0 * 2 * pps, pps);
    mp.use_add_tab = !q.fold;
    mp.add_tab = c0;
    switch_key_mod_down(c, l, q, mp);
  }
  // (ct_views with a batch per handle)
  size_t at = 0;
  for (uint32_t i = 0; i < n_handles; i++) {
    evah_ct *t = new evah_ct;
    t->buf = ob.b;
    t->d = ob.b->d + at * 2 * pps;
    t->size = 2, t->limbs = l, t->ps = pps;
    t->scale = cts[i]->scale;
    t->batch = cts[i]->batch;
    outs[i] = t;
    at += cts[i]->batch;
  }
  ob.b->refs = (int)n_handles;
  ob.b = nullptr;
  API_END
}

// a batched handle is batch * size polynomials at stride ps (more than a PtrTab holds: evah_rescale_many's tables do not apply)
int evah_rescale(evah_ctx *c, const evah_ct *a, uint32_t divisor_bits, evah_ct **out) {
  API_BEGIN
  use(c);
  acquire(c, a->buf);
  if (a->limbs < 2) throw std::invalid_argument("end of modulus switching chain reached");
  const uint32_t l = a->limbs, polys = a->size * a->batch;
  const size_t N = c->N, ops = (size_t)(l - 1) * N;
  FreshBuf ob(c, (size_t)polys * ops);
  Scratch r(c, (size_t)polys * N);
  OpPlain::Params ip{a->d + (size_t)(l - 1) * N, r.d, a->ps, N, 1, l - 1, 1, {}};
  OpModDown::Params mp{r.d, N, a->d, a->ps, nullptr, 0, 0, ob.d(), ops, l - 1, l - 1};
  inverse_then_forward<OpPlain, OpModDown>(c, ip, polys, mp, polys * (l - 1));
  ct_views(c, ob, 1, a->size, l - 1, a->batch, [&](uint32_t) { return a->scale / pow2(divisor_bits); }, out);
  API_END
}

} // extern "C"
