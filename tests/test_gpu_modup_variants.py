"""Every instantiation of the key switch's mod-up kernel (ntt_modup_kernel) leaves the same words.

The kernel has two shapes behind EVAH_MODUP_LR, both on 2048-coefficient tiles (3: 8 coefficients per thread, 256
threads; 2: 4 per thread, 512 threads) and three bodies chosen from the context's primes (Context.modup_variant()):
  fully specialised  every prime of the top-bit shape and q_J <= 8 q_kappa for every digit / output prime pair: top-bit
                     butterflies only, lazy digit conversion only;
  top-bit only       every prime of the top-bit shape, some q_J > 8 q_kappa: both conversions compiled in;
  generic            some prime of another shape — or EVAH_MODUP_SPEC=0 on any chain.
Each case below gives the same keys and operands to contexts that differ only in these knobs.  Every result must be the
oracle's words and, word for word, what a context with EVAH_MODUP=0 (the two-launch form) returns; the case's reference
words are computed once and shared by its variants.  EVAH_FUSE_SMALL=0 pushes the small shapes past the fused small-launch
form, and a launch count (the stand-alone strided inverse pass of the digits is gone, no other count moves) proves that
the mod-up kernel is what ran, so no comparison is vacuous.  Cases:
  N = 2^11 (P = 6), l = 3, 60-bit primes: ONE column tile per digit, so the digit index is the whole of blockIdx.x (every
      other case has more, the tile in its low bits), on the fully specialised kernel;
  N = 2^12, l = 3, 60-bit and 38 / 40-bit primes: all top-bit, q_J > 8 q_kappa for the 60-bit digits under the small primes,
      so the kernel is top-bit only and the canonical conversion is hit;
  N = 2^12 with a 55-bit prime of no top-bit shape: the generic kernel at both LR, whatever EVAH_MODUP_SPEC says;
  N = 2^13 (P = 7) and N = 2^15 (P = 8, the headline's), l = 2, fully specialised;
  worst-case words at N = 2^12 — every residue q - 1 (and every coefficient q - 1), keys at q - 1 — on the 60-bit chain and
      on the mixed one: the lazy-bound edges of test_gpu_extremes.py on every variant."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

VARIANTS = [(lr, spec) for lr in (3, 2) for spec in (1, 0)]


def _ctx(N, primes, knobs):
    env = dict(knobs, EVAH_FUSE_SMALL=0)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return backend.Context(N, primes)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ntt_prime_below(bound, N):
    q = bound - (bound % (2 * N)) + 1
    while q >= bound or not po.lib.evo_is_prime(q):
        q -= 2 * N
    return q


def _nontb_chain(N):
    c60 = po.coeff_modulus_create(N, [60] * 5)
    nontb = _ntt_prime_below((1 << 55) - (1 << 40), N)  # 2^55 - c with c >= 2^32, above 2^54: no top-bit shape
    return [c60[0], nontb, c60[1], c60[4]]


# name -> (N, primes, (top-bit only, lazy only) of the specialised kernel, operand kind)
CASES = {
    "N2048_60x4": lambda: (1 << 11, po.coeff_modulus_create(1 << 11, [60] * 4), (True, True), "random"),
    "N4096_mixed": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60, 38, 60, 40]), (True, False), "random"),
    "N4096_nontb55": lambda: (1 << 12, _nontb_chain(1 << 12), (False, False), "random"),
    "N8192_60x3": lambda: (1 << 13, po.coeff_modulus_create(1 << 13, [60] * 3), (True, True), "random"),
    "N32768_60x3": lambda: (1 << 15, po.coeff_modulus_create(1 << 15, [60] * 3), (True, True), "random"),
    "N4096_60x4_qm1": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60] * 4), (True, True), "qm1"),
    "N4096_60x4_dense_max": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60] * 4), (True, True), "dense_max"),
    "N4096_mixed_qm1": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60, 38, 60, 40]), (True, False), "qm1"),
    "N4096_mixed_dense_max": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60, 38, 60, 40]), (True, False), "dense_max"),
}


class _Case:
    """keys, operands, the oracle's words and the EVAH_MODUP=0 context's words and launch counts of one case"""

    def __init__(self, name):
        self.N, self.primes, self.spec_flags, kind = CASES[name]()
        N, primes = self.N, self.primes
        k = len(primes)
        l = self.l = k - 1
        self.div = int(primes[-2]).bit_length()
        o = po.Oracle(N, primes)
        rng = np.random.default_rng(N + k)

        def rand(prefix, nl):
            return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))
        if kind == "random":
            self.rk = rand((l, 2), k)
            self.ops = [(rand((2,), l), rand((2,), l)) for _ in range(2)]
            self.m = o.multiply(*self.ops[0])
        else:  # worst-case words: keys at q - 1; every residue (qm1) / every coefficient (dense_max) at q - 1
            self.rk = np.stack([np.full((l, 2, N), primes[i] - 1, dtype=np.uint64) for i in range(k)], axis=2)
            if kind == "qm1":
                p = np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])
            else:
                p = np.stack([o.ntt(i, np.full(N, primes[i] - 1, dtype=np.uint64)) for i in range(l)])
            self.ops = [(np.stack([p, p]), np.stack([p, p]))] * 2
            self.m = np.stack([p, p, p])  # the key-switch target is the worst-case polynomial itself
        relin = o.relinearize(self.m, self.rk)
        self.want = [o.op_triple(a, b, self.rk) for a, b in self.ops] + [relin, o.rescale(relin)]
        g = _ctx(N, primes, {"EVAH_MODUP": 0})
        try:
            self.ref = self.run(g)
            self.ref_launches = self.launches(g)
        finally:
            g.close()
        for got, want in zip(self.ref, self.want):
            assert np.array_equal(got, want), "EVAH_MODUP=0 differs from the oracle"

    def run(self, g):
        """2 fused op-triples in one call, relinearize and relinearize + rescale of a stored product"""
        g.upload_relin_key(self.rk)
        up = [(g.upload_ct(a, 2.0 ** 30), g.upload_ct(b, 2.0 ** 30)) for a, b in self.ops]
        out = [c.download() for c in g.multiply_relinearize_rescale_many([u[0] for u in up], [u[1] for u in up], self.div)]
        M = g.upload_ct(self.m, 2.0 ** 60)
        return out + [g.relinearize(M).download(), g.relinearize_rescale(M, self.div).download()]

    def launches(self, g):
        """{kernel class: launches} of one relinearize of the stored product"""
        M = g.upload_ct(self.m, 2.0 ** 60)
        g.profile(True)
        g.profile_reset()
        keep = g.relinearize(M)
        g.sync()
        del keep
        n = {name: cnt for name, (cnt, _) in g.profile_get().items()}
        g.profile(False)
        return n


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = _Case(name)
    return _CACHE[name]


@pytest.mark.parametrize("lr,spec", VARIANTS, ids=[f"lr{lr}_spec{spec}" for lr, spec in VARIANTS])
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_variant_leaves_the_same_words(name, lr, spec):
    c = _case(name)
    g = _ctx(c.N, c.primes, {"EVAH_MODUP": 1, "EVAH_MODUP_LR": lr, "EVAH_MODUP_SPEC": spec})
    try:
        # the instantiation the context chose: the shape asked for, the specialisation its primes allow
        assert g.modup_variant() == ((lr,) + c.spec_flags if spec else (lr, False, False))
        got = c.run(g)
        for i, (x, ref, want) in enumerate(zip(got, c.ref, c.want)):
            assert np.array_equal(x, ref), f"result {i}: EVAH_MODUP=1 and EVAH_MODUP=0 differ"
            assert np.array_equal(x, want), f"result {i}: differs from the oracle"
        # the mod-up kernel is what ran: the digits' stand-alone strided inverse pass is gone, into the ksdigit_pass1
        # launch the key switch had anyway; no other count moves
        n = c.launches(g)
        assert c.ref_launches["intt_pass2"] >= 1 and c.ref_launches["ksdigit_pass1"] >= 1, c.ref_launches
        assert n == dict(c.ref_launches, intt_pass2=c.ref_launches["intt_pass2"] - 1), (n, c.ref_launches)
    finally:
        g.close()


def test_default_shape_is_one_of_the_two():
    """without the knobs a 60-bit chain takes the fully specialised kernel at the default shape"""
    N = 1 << 11
    g = _ctx(N, po.coeff_modulus_create(N, [60] * 4), {})
    try:
        lr, tb, lazy = g.modup_variant()
        assert lr in (2, 3) and tb and lazy
    finally:
        g.close()
