"""The three-launch tail of relinearize + rescale (EVAH_TAIL_FUSE=1: OpTailIntt, ntt_tail_kernel, OpRRT's contiguous pass)
leaves the words of the six-launch tail (EVAH_TAIL_FUSE=0) and of the oracle.

The fused tail runs where the key switch takes the mod-up kernel, so EVAH_FUSE_SMALL=0 pushes the small shapes here past the
small-launch form, as the mod-up variant tests do.  Each case gives the same keys and operands to two contexts that differ
in EVAH_TAIL_FUSE only and compares, word for word, the fused op-triple (multiply_relinearize_rescale_many with 1 and with 3
products, and on a batched handle) and relinearize_rescale of a stored product (single, _many with 3 handles, a batched
handle); the six-launch context's words are the oracle's.  Launch counts of one relinearize_rescale and one op-triple call
prove which tail ran: the six-launch tail has two strided inverse launches (intt_pass2: the special rows', the last rows')
and two contiguous ones, the fused tail no strided inverse launch at all and one contiguous one; no other count moves.
Cases:
  N = 2^12 (passes 6, 6) and N = 2^13 (7, 6: the odd split), four 60-bit primes: the fully specialised kernel;
  the nontb55 chain of test_gpu_extremes.py (a 55-bit prime of no top-bit shape) at both N: the generic kernel;
  N = 2^12 with 60, 38, 60-bit data primes and a 40-bit special prime: all top-bit, q_last > 4 q_i for the 38-bit prime, so
      the kernel is top-bit only and takes the canonical conversion on that row;
  operands: uniform random words; every residue at q - 1 (qm1) and every coefficient of limb J at q_J - 1 (dense_max: every
      digit at its prime's maximum), with keys at q - 1 — the worst-case words of test_gpu_extremes.py."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


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


def _nontb55(N):
    c60 = po.coeff_modulus_create(N, [60] * 5)
    nontb = _ntt_prime_below((1 << 55) - (1 << 40), N)  # 2^55 - c with c >= 2^32, above 2^54: no top-bit shape
    return [c60[0], nontb, c60[1], c60[4]]


# name -> (N, primes, (top-bit only, lazy only) of the tail kernel, operand kind)
CASES = {
    "N4096_60x4": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60] * 4), (True, True), "random"),
    "N4096_60x4_qm1": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60] * 4), (True, True), "qm1"),
    "N4096_60x4_dense_max": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60] * 4), (True, True), "dense_max"),
    "N8192_60x4": lambda: (1 << 13, po.coeff_modulus_create(1 << 13, [60] * 4), (True, True), "random"),
    "N8192_60x4_dense_max": lambda: (1 << 13, po.coeff_modulus_create(1 << 13, [60] * 4), (True, True), "dense_max"),
    "N4096_nontb55": lambda: (1 << 12, _nontb55(1 << 12), (False, False), "random"),
    "N4096_nontb55_qm1": lambda: (1 << 12, _nontb55(1 << 12), (False, False), "qm1"),
    "N8192_nontb55": lambda: (1 << 13, _nontb55(1 << 13), (False, False), "random"),
    "N4096_mixed": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60, 38, 60, 40]), (True, False), "random"),
    "N4096_mixed_dense_max": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60, 38, 60, 40]), (True, False), "dense_max"),
}


class _Case:
    """keys, operands, the oracle's words, and the EVAH_TAIL_FUSE=0 context's words and launch counts of one case"""

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
            self.ops = [(rand((2,), l), rand((2,), l)) for _ in range(3)]
            self.m = o.multiply(*self.ops[0])
        else:  # worst-case words: keys at q - 1; every residue (qm1) / every coefficient (dense_max) at q - 1
            self.rk = np.stack([np.full((l, 2, N), primes[i] - 1, dtype=np.uint64) for i in range(k)], axis=2)
            if kind == "qm1":
                p = np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])
            else:
                p = np.stack([o.ntt(i, np.full(N, primes[i] - 1, dtype=np.uint64)) for i in range(l)])
            self.ops = [(np.stack([p, p]), np.stack([p, p]))] * 3
            self.m = np.stack([p, p, p])  # the key-switch target is the worst-case polynomial itself
        triples = [o.op_triple(a, b, self.rk) for a, b in (self.ops if kind == "random" else self.ops[:1])]
        if kind != "random":
            triples = triples * 3
        rr = o.rescale(o.relinearize(self.m, self.rk))
        # in the order of run(): op-triple of 1, of 3, batched (instances 0 and 1); relinearize_rescale single, x3, batched x2
        self.want = [triples[0]] + triples + triples[:2] + [rr] * 6
        g = _ctx(N, primes, {"EVAH_TAIL_FUSE": 0})
        try:
            assert g.tail_variant()[0] is False
            self.ref = self.run(g)
            self.ref_launches = self.launches(g)
        finally:
            g.close()
        assert len(self.ref) == len(self.want)
        for i, (got, want) in enumerate(zip(self.ref, self.want)):
            assert np.array_equal(got, want), f"result {i}: EVAH_TAIL_FUSE=0 differs from the oracle"

    def _upload(self, g):
        g.upload_relin_key(self.rk)
        up = [(g.upload_ct(a, 2.0 ** 30), g.upload_ct(b, 2.0 ** 30)) for a, b in self.ops]
        M = g.upload_ct(self.m, 2.0 ** 60)
        return up, M

    def run(self, g):
        up, M = self._upload(g)
        A, B = [u[0] for u in up], [u[1] for u in up]
        out = [c.download() for c in g.multiply_relinearize_rescale_many(A[:1], B[:1], self.div)]
        out += [c.download() for c in g.multiply_relinearize_rescale_many(A, B, self.div)]
        AB = [g.upload_ct_batch(np.stack([self.ops[0][x], self.ops[1][x]]), 2.0 ** 30) for x in (0, 1)]
        out += list(g.multiply_relinearize_rescale(AB[0], AB[1], self.div).download())
        out.append(g.relinearize_rescale(M, self.div).download())
        out += [c.download() for c in g.relinearize_rescale_many([M, M, M], self.div)]
        M2 = g.upload_ct_batch(np.stack([self.m, self.m]), 2.0 ** 60)
        out += list(g.relinearize_rescale(M2, self.div).download())
        return out

    def launches(self, g):
        """{kernel class: launches} of one relinearize_rescale of the stored product and of one op-triple call of 3"""
        up, M = self._upload(g)
        counts = []
        for call in (lambda: g.relinearize_rescale(M, self.div),
                     lambda: g.multiply_relinearize_rescale_many([u[0] for u in up], [u[1] for u in up], self.div)):
            g.profile(True)
            g.profile_reset()
            keep = call()
            g.sync()
            del keep
            counts.append({name: cnt for name, (cnt, _) in g.profile_get().items()})
            g.profile(False)
        return counts


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        _CACHE[name] = _Case(name)
    return _CACHE[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_tail_leaves_the_same_words(name):
    c = _case(name)
    g = _ctx(c.N, c.primes, {"EVAH_TAIL_FUSE": 1})
    try:
        assert g.tail_variant() == (True,) + c.spec_flags
        got = c.run(g)
        assert len(got) == len(c.ref)
        for i, (x, ref, want) in enumerate(zip(got, c.ref, c.want)):
            assert np.array_equal(x, ref), f"result {i}: EVAH_TAIL_FUSE=1 and EVAH_TAIL_FUSE=0 differ"
            assert np.array_equal(x, want), f"result {i}: differs from the oracle"
        # the three-launch tail is what ran: both strided inverse launches and one contiguous inverse launch are gone,
        # the strided forward launch (moddown_pass1) is the tail kernel; no other count moves
        for n, ref in zip(c.launches(g), c.ref_launches):
            assert ref["intt_pass2"] == 2 and ref["moddown_pass1"] == 1 and ref["moddown_pass2"] == 1, ref
            assert n == dict(ref, intt_pass1=ref["intt_pass1"] - 1, intt_pass2=0), (n, ref)
    finally:
        g.close()


def test_generic_kernel_on_a_chain_that_allows_the_specialised_one():
    """EVAH_MODUP_SPEC=0 selects the generic tail kernel on 60-bit primes: same words"""
    c = _case("N4096_60x4")
    g = _ctx(c.N, c.primes, {"EVAH_TAIL_FUSE": 1, "EVAH_MODUP_SPEC": 0})
    try:
        assert g.tail_variant() == (True, False, False)
        for i, (x, ref) in enumerate(zip(c.run(g), c.ref)):
            assert np.array_equal(x, ref), f"result {i}"
    finally:
        g.close()


def test_the_knob_is_on_by_default():
    N = 1 << 12
    g = _ctx(N, po.coeff_modulus_create(N, [60] * 4), {})
    try:
        assert g.tail_variant() == (True, True, True)
    finally:
        g.close()
