// ntt_tail.hip.h — the tail of relinearize + rescale at throughput size: ntt_tail_kernel
// (included by ntt.hip.h after ntt_modup.hip.h, whose structure it mirrors)
#pragma once
#include "ntt.hip.h"

namespace evah {

// The strided passes of the relinearize + rescale tail (RR_FOLDED form), one workgroup per (2048-coefficient column tile,
// polynomial = 2 b + K).  The six-launch tail finishes r_K = INTT_P(special row) + P/2 and stores it, finishes
// t_K = INTT_last(prod P^-1) - u P^-1 + q_last/2 (OpRRLastT::store, which reads r_K) and stores it, and then reads both
// once per output prime in OpRRT's strided pass.  r_K and t_K at a coefficient are functions of the two inverse tiles at
// that coefficient only, so here the workgroup
//   1. runs the strided inverse pass of the special-row tile (from the contiguous inverse pass's intermediate in lp.r,
//      N^-1 folded in) and keeps the canonical r_K (+ P/2, OpPlain's epilogue) in registers; the last-row tile and its
//      inverse twiddles are requested before these rounds and land during them;
//   2. runs the strided inverse pass of the last-row tile (intermediate in lp.t) and forms t_K = OpRRLastT::combine in
//      registers — the same thread holds both tiles' words of a coefficient;
//   3. walks the output primes i = 0 .. rp.jl - 1: OpRRT::conv<LZ> from the registers, the strided forward rounds, and
//      the lazy first-pass words to rp.dst[poly][i] — what OpRRT's strided pass writes, at the same place, so OpRRT's
//      contiguous pass follows unchanged.  Row i + 1's twiddles and constants are requested before row i's butterflies.
// r_K and t_K never reach memory.  Tile geometry, twiddle staging and the row stores through one buffer descriptor per
// row are ntt_modup_kernel's at 8 coefficients per thread (256 threads): LDS holds the tile and 2^P twiddles.
// Lazy bound of step 3 (OpRRT::setup): with q_last <= 4 q_i and P <= 8 q_i, conv<true> = lazy5(r + q_i - halfP) +
// t + q_i - halfL < 5 q_i + q_last + q_i <= 10 q_i, inside the < 12 q_i the first forward pass accepts (ntt_round: it
// reduces on the stages tb_reduce_stage / RED_EVEN = false name and leaves < 16 q_i); a prime that fails the test takes
// conv<false>, canonical.  As in the mod-up two facts about the context's primes, established once on the host
// (evah_ctx::modup_tb / tail_lazy), each remove a code path from the row loop:
//   TBONLY    every prime has the top-bit shape: the forward rounds are the top-bit RoundSeq only
//   LAZYONLY  the test above holds for every (last, i) pair of every level: only conv<true> is instantiated
// grid = (n_tiles, 1, polys), block = 256.
template <int P, bool TBONLY = false, bool LAZYONLY = false>
__global__ void __launch_bounds__(NTT_THREADS)
ntt_tail_kernel(DevCtx cx, OpRRLastFolded::Params lp, OpRRFolded::Params rp) {
  extern __shared__ __attribute__((aligned(16))) u64 lds[];
  constexpr int LR = 3, NTT_R = 1 << LR, T = NTT_THREADS;
  constexpr int S = 1 << P, TPS = S / NTT_R, SP = lds_sub_stride<P>();
  constexpr int logC = 8 + LR - P, C = 1 << logC;
  constexpr int TWR = (S + T - 1) / T; // twiddles staged per thread
  if (cx.skipped()) return;
  const uint32_t tile_idx = blockIdx.x, poly = blockIdx.z;
  OpRRLastFolded::Job jl;
  OpRRLastFolded::setup(cx, lp, 0, poly, 0, jl);
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
  ulonglong2 *twl = reinterpret_cast<ulonglong2 *>(lds + ((C * SP + 1) & ~1));
  ulonglong2 twn[TWR]; // the next transform's twiddles, on their way from memory
  auto tw_request = [&](const ulonglong2 *table, uint32_t prime) {
    const ulonglong2 *tw = table + (size_t)prime * cx.N;
#pragma unroll
    for (int r = 0; r < TWR; r++)
      if (S >= T || (int)threadIdx.x + r * T < S) twn[r] = tw[threadIdx.x + r * T];
  };
  auto tw_stage = [&]() {
#pragma unroll
    for (int r = 0; r < TWR; r++)
      if (S >= T || (int)threadIdx.x + r * T < S) twl[threadIdx.x + r * T] = twn[r];
  };
  const int sub = threadIdx.x / TPS, tid = threadIdx.x % TPS;
  u64 r[NTT_R], t[NTT_R]; // this thread's words of r_K and t_K: every output row converts them from here
  // the uniform round's twiddles (UTw, ntt.hip.h) of the transform at hand, in scalar registers straight from the
  // tables: requested before the barrier in front of its rounds (a transform ahead, two sets are live across the
  // butterflies and the kernel spills scalar registers: profiles/r11_tw_sgpr_notes.md)
  UTwOf<P, LR> ut;
  {
    // ---- 1. the special-row tile modulo P
    const DevPrime pmP = cx.primes[lp.sp];
    const u64 *srcP = jl.r, *srcL = jl.dst;
    tw_request(cx.tw_inv, lp.sp);
    utw_load(ut, cx.tw_inv, lp.sp, cx.N, 2);
#pragma unroll
    for (int it = 0; it < NTT_R; it++) lds[lds_at(it)] = srcP[n0 + it * nstep];
    tw_stage();
#pragma unroll
    for (int it = 0; it < NTT_R; it++) t[it] = srcL[n0 + it * nstep]; // the last-row tile, in flight during the rounds below
    tw_request(cx.tw_inv, jl.prime);
    __syncthreads();
    RoundSeq<P, LR, 0, true, true, false>::run(lds + sub * SP, tid, 0, 0, twl, pmP, ut); // canonical mod P (N^-1 folded in)
    __syncthreads();
    // every thread is past the rounds: the twiddle buffer and the tile may be rewritten; each thread rewrites only the
    // tile slots it reads here
#pragma unroll
    for (int it = 0; it < NTT_R; it++) {
      r[it] = addmod(lds[lds_at(it)], pmP.q >> 1, pmP.q);
      lds[lds_at(it)] = t[it];
    }
    tw_stage();
  }
  typename OpRRFolded::Job jb;
  uint32_t iy = 0;
  OpRRFolded::setup(cx, rp, 0, iy, poly, jb);
  tw_request(cx.tw_fwd, jb.prime);
  utw_load(ut, cx.tw_inv, jl.prime, cx.N, 2);
  __syncthreads();
  {
    // ---- 2. the last-row tile modulo q_last, t_K
    const DevPrime pmL = cx.primes[jl.prime];
    RoundSeq<P, LR, 0, true, true, false>::run(lds + sub * SP, tid, 0, 0, twl, pmL, ut); // canonical mod q_last
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NTT_R; it++) t[it] = OpRRLastFolded::combine(jl, pmL, lds[lds_at(it)], r[it]);
  }
  // ---- 3. every output prime
  while (true) {
    // every thread is past the previous rounds (barrier above / below)
    tw_stage();
    // the row's prime, its uniform twiddles and the conversion's constants: scalar loads, waited for once
    const DevPrime pm = pass_prime(cx, jb.prime);
    utw_load(ut, cx.tw_fwd, jb.prime, cx.N);
#if EVAH_TW_SGPR
    OpRRFolded::conv_consts_uniform(cx, rp, jb);
#endif
    auto convert = [&](auto lazy_tag) {
      constexpr bool LZ = decltype(lazy_tag)::value;
#pragma unroll
      for (int it = 0; it < NTT_R; it++) lds[lds_at(it)] = OpRRFolded::template conv<LZ>(jb, pm, r[it], t[it]);
    };
    if (LAZYONLY || jb.lazy) convert(std::true_type{});
    else if constexpr (!LAZYONLY) convert(std::false_type{});
    // the next row's twiddles are in flight during this row's butterflies
    typename OpRRFolded::Job jn;
    const bool more = iy + 1 < rp.jl;
    if (more) {
      OpRRFolded::setup(cx, rp, 0, iy + 1, poly, jn);
      tw_request(cx.tw_fwd, jn.prime);
    }
    __syncthreads();
    if constexpr (TBONLY) RoundSeq<P, LR, 0, false, true, false, true, true>::run(lds + sub * SP, tid, 0, 0, twl, pm, ut);
    else forward_rounds<P, LR, true, false>(lds + sub * SP, tid, 0, 0, twl, pm, ut);
    __syncthreads();
    // a row is at most 2^17 * 8 bytes: offsets fit 32 bits
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
    iy++;
  }
}

} // namespace evah
