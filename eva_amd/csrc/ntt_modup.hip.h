// ntt_modup.hip.h — the key switch's mod-up at throughput size: ntt_modup_kernel
// (included by ntt.hip.h beside ntt_inv_fwd_kernel, whose hooks it shares)
#pragma once
#include "ntt.hip.h"

namespace evah {

// Strided inverse pass of one digit + digit conversion and forward strided pass under EVERY output prime, one workgroup per
// (column tile, digit J, instance b).  ntt_inv_fwd_kernel does the same per (I, J) job and so recomputes the inverse tile
// for each of the l + 1 output rows, which only pays while the launch is far from filling the chip; here the tile is
// inverted once (from the contiguous inverse pass's intermediate in Op::pre_src, N^-1 folded in), its canonical words
// t_J stay in registers, and the workgroup walks the output rows I = 0 .. prm.ni - 1 of Op::setup (I == J has no job)
// converting t_J (Op::conv) and running the forward strided rounds into scratch[b][I][J] — the same lazy intermediate,
// at the same place, as the two-launch form (inverse strided pass storing t, then the OpKsDigit strided pass reading
// it once per output row).  t never reaches memory, and the digit tile is read once instead of l times.
// Each row's forward twiddles are requested during the previous row's butterflies and staged in the one twiddle
// buffer once those are done: LDS holds the tile and 2^P twiddles, as the stand-alone strided pass.
// grid = (n_tiles * l, 1, batch) with the tile in the low log_tiles bits of x, block = NT, tile = NT << LR.
// The host launches LR = 3 on 256 threads or LR = 2 on 512 (a fourth LDS round trip per pass at P = 8, fewer registers):
// either way a 2048-coefficient tile whose row segments are 2^(11 - P) words (launch_modup_v, launch.hip.h).
// The row loop is what decides the kernel's registers, and with them the waves per SIMD.  Two facts about a context's
// primes, established once on the host (evah_ctx::modup_tb / modup_lazy), each remove a code path that would otherwise
// be live beside the one taken:
//   TBONLY    every prime has the top-bit shape (DevPrime::tb_c != 0): the forward rounds are the top-bit RoundSeq, no
//             block-uniform choice between it and the compare-and-subtract family
//   LAZYONLY  q_J <= 8 q_kappa for every digit / output prime pair: only Op::conv<true> is instantiated (jb.lazy holds
//             for every job)
// A context that fails either test runs the generic instantiation; all of them leave the same words.
// A row's words leave through ONE buffer descriptor on the row's (workgroup-uniform) base: the per-thread part of the
// address is a single 32-bit offset (8 n0) and the per-element part a scalar offset (8 it nstep), where flat stores made
// the compiler keep 2^LR 64-bit addresses live across the row loop.  A row is at most 2^17 * 8 bytes: offsets fit 32 bits.
// NT = threads per workgroup (this kernel only): the tile is NT << LR coefficients, 2^(log2 NT + LR - P) columns wide.
template <int P, int LR, class Op, bool TBONLY = false, bool LAZYONLY = false, int NT = NTT_THREADS>
__global__ void __launch_bounds__(NT)
ntt_modup_kernel(DevCtx cx, typename Op::Params prm, int log_tiles) {
  static_assert(NT == 256 || NT == 512, "ntt_modup_kernel: 256 or 512 threads");
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  constexpr int NTT_R = 1 << LR;
  constexpr int S = 1 << P, TPS = S / NTT_R, SP = lds_sub_stride<P>();
  constexpr int logC = (NT == 512 ? 9 : 8) + LR - P, C = 1 << logC, T = NT;
  constexpr int TWR = (S + T - 1) / T; // twiddles staged per thread
  if (cx.skipped()) return;
  const uint32_t tile_idx = blockIdx.x & ((1u << log_tiles) - 1u), J = blockIdx.x >> log_tiles, b = blockIdx.z;
  // first output row with a job (block-uniform)
  typename Op::Job jb;
  uint32_t iy = 0;
  while (iy < prm.ni && !Op::setup(cx, prm, J, iy, b, jb)) iy++;
  if (iy >= prm.ni) return;
  const uint32_t pa = Op::pre_prime(prm, jb);
  const DevPrime pmA = cx.primes[pa];
  const uint32_t stride_log = cx.logN - P;
  constexpr int ES = 1 << (P - LR);
  constexpr bool LINEAR = (ES % 16 == 0);
  const int c = threadIdx.x & (C - 1), e0 = threadIdx.x >> logC;
  const uint32_t n0 = (tile_idx << logC) + ((uint32_t)e0 << stride_log) + c, nstep = (uint32_t)(T >> logC) << stride_log;
  const int l0 = c * SP + lds_pad<P>(e0);
  auto lds_at = [&](int it) -> int {
    if constexpr (LINEAR) return l0 + it * lds_pad<P>(ES);
    const int idx = threadIdx.x + it * T;
    return (idx & (C - 1)) * SP + lds_pad<P>(idx >> logC);
  };
  const u64 *src = Op::pre_src(jb);
#pragma unroll
  for (int it = 0; it < NTT_R; it++) lds[lds_at(it)] = src[n0 + it * nstep];
  ulonglong2 *twl = reinterpret_cast<ulonglong2 *>(lds + ((C * SP + 1) & ~1));
  const ulonglong2 *twA = cx.tw_inv + (size_t)pa * cx.N;
  for (int idx = threadIdx.x; idx < S; idx += T) twl[idx] = twA[idx];
  ulonglong2 twn[TWR]; // the next output row's forward twiddles, on their way from memory
  auto tw_request = [&](uint32_t prime) {
    const ulonglong2 *tw = cx.tw_fwd + (size_t)prime * cx.N;
#pragma unroll
    for (int r = 0; r < TWR; r++)
      if (S >= T || (int)threadIdx.x + r * T < S) twn[r] = tw[threadIdx.x + r * T];
  };
  tw_request(jb.prime);
  // the uniform round's twiddles (UTw, ntt.hip.h) go to scalar registers straight from the tables: here the inverse
  // pass's last round; each row's first forward round in the row loop
  UTwOf<P, LR> utA;
  utw_load(utA, cx.tw_inv, pa, cx.N, 2);
  __syncthreads();
  const int sub = threadIdx.x / TPS, tid = threadIdx.x % TPS;
  RoundSeq<P, LR, 0, true, true, false>::run(lds + sub * SP, tid, 0, 0, twl, pmA, utA); // canonical mod q_J (N^-1 folded in)
  __syncthreads();
  u64 t[NTT_R]; // this thread's words of t_J: every output row converts them from here
#pragma unroll
  for (int it = 0; it < NTT_R; it++) {
    t[it] = lds[lds_at(it)];
    if (Op::pre_addhalf) t[it] = addmod(t[it], pmA.q >> 1, pmA.q);
  }
  while (true) {
    // every thread is past the previous row's rounds (barrier below): the twiddle buffer and the tile may be rewritten;
    // each thread rewrites only the tile slots it stored from itself
#pragma unroll
    for (int r = 0; r < TWR; r++)
      if (S >= T || (int)threadIdx.x + r * T < S) twl[threadIdx.x + r * T] = twn[r];
    // the row's prime and its uniform twiddles: scalar loads, waited for once, before the conversion.  (Requested a row
    // ahead, beside tw_request below, two sets of 28 scalar registers are live across the butterflies and the kernels
    // spill scalar registers: profiles/r11_tw_sgpr_notes.md)
    const DevPrime pm = pass_prime(cx, jb.prime);
    UTwOf<P, LR> ut;
    utw_load(ut, cx.tw_fwd, jb.prime, cx.N);
    auto convert = [&](auto lazy_tag) {
      constexpr bool LZ = decltype(lazy_tag)::value;
#pragma unroll
      for (int it = 0; it < NTT_R; it++) lds[lds_at(it)] = Op::template conv<LZ>(jb, pm, t[it]);
    };
    if (LAZYONLY || jb.lazy) convert(std::true_type{});
    else if constexpr (!LAZYONLY) convert(std::false_type{});
    // next row with a job (block-uniform); its twiddles are in flight during this row's butterflies
    typename Op::Job jn;
    uint32_t in = iy + 1;
    while (in < prm.ni && !Op::setup(cx, prm, J, in, b, jn)) in++;
    const bool more = in < prm.ni;
    if (more) tw_request(jn.prime);
    __syncthreads();
    if constexpr (TBONLY) RoundSeq<P, LR, 0, false, true, false, true, true>::run(lds + sub * SP, tid, 0, 0, twl, pm, ut);
    else forward_rounds<P, LR, true, false>(lds + sub * SP, tid, 0, 0, twl, pm, ut);
    __syncthreads();
    const __amdgpu_buffer_rsrc_t row = __builtin_amdgcn_make_buffer_rsrc(jb.dst, 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int it = 0; it < NTT_R; it++) { // lazy intermediate of the forward transform, at jb.dst[n0 + it * nstep]
      typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
      const u64 v = lds[lds_at(it)];
      u32x2 w;
      w.x = (uint32_t)v;
      w.y = (uint32_t)(v >> 32);
      __builtin_amdgcn_raw_buffer_store_b64(w, row, 8u * n0, 8u * (uint32_t)it * nstep, 0);
    }
    if (!more) break;
    jb = jn;
    iy = in;
  }
}

} // namespace evah
