"""The digit loop of the one-wave radix-2^30 key-switch kernel (ks_inner_kernel<MAC3>; EVAH_KS_LOOP, ntt_ks_inner.hip.h) —
sums that accumulate in their own registers, the top-bit constant as a scalar factor, the first contiguous round's
workgroup-uniform twiddles from scalar registers — leaves the oracle's words, in every epilogue the kernel has.

Nothing the loop computes may move: same products, same order of additions, same residues.  So every case compares with
the CPU oracle word for word, and the launch counts per kernel class are the ones the launch layer issued before the loop
changed (the tables below; the host code is untouched, the counts say that the kernels under test are what ran).

The throughput forms are forced on at these small launch sizes (EVAH_MODUP=1, and EVAH_FUSE_SMALL=0, which keeps the
small-launch form away), as in test_gpu_ks_tail.py.
Degrees (the kernel is compiled per contiguous pass size P):
  N = 2^12  passes (6, 6): four sub-transforms per 256-coefficient tile;
  N = 2^13  (7, 6);
  N = 2^15  (8, 7): P = 7, two sub-transforms per tile — the instantiation of the Harris leg;
  N = 2^16  (8, 8): P = 8, ONE sub-transform per tile — the only size at which the first round's twiddles are uniform
            and come from scalar registers (the digits and slice B's correction tile; the stored-product kernel too).
Limb counts, by where the loop can go wrong (all 60-bit primes; the deep ones at N = 2^12 only):
  l = 2   no fold of the sums, the shortest loop (slice B is one row);
  l = 3   (N = 2^13);
  l = 7   MAC3_FOLD_DIGITS is reached on the last digit: no fold;
  l = 8   exactly one mac3_fold;
  l = 15  two folds; the largest l the radix-2^30 kernel is selected for (MAC3_MAX_LIMBS).
Chains: 60/38/60/40 (top-bit shape with small primes); nontb55 (a 55-bit prime of no top-bit shape: the 128-bit kernel, a
launch form that must be unchanged in counts and words).
Words: uniform random; every residue at q - 1 (qm1); every coefficient of limb J at q_J - 1 (dense_max); keys at q - 1 for
the latter two — the generators of the neighbouring tests.
Calls: relinearize (KS_FOLDADD, no tail epilogue: prod is stored);
relinearize_rescale (KS_FOLDADD) and multiply_relinearize_rescale_many of 1 and 3 products (KS_FOLDMUL) with EVAH_KS_TAIL=0
(KS_TAIL_NONE) and =1 (slices A and B); one rotation (KS_FOLDADD with the permuted c0 added to polynomial 0 only)."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

STEP = 3
ZERO = {"elementwise": 0, "intt_pass1": 0, "intt_pass2": 0, "ksdigit_pass1": 0, "ksdigit_pass2": 0, "ks_mac": 0,
        "moddown_pass1": 0, "moddown_pass2": 0, "ntt_pass1": 0, "ntt_pass2": 0}
# launches per kernel class of one call's launch set, radix-2^30 contexts.  relinearize + rescale of a stored product and
# the op-triple (whose product is formed by one more inverse pass): the three-launch tail, and with the tail's contiguous
# passes inside the two key-switch slices (test_gpu_ks_tail.py's tables)
RR_TAIL0 = dict(ZERO, intt_pass1=2, ksdigit_pass1=1, ks_mac=1, moddown_pass1=1, moddown_pass2=1)
RR_TAIL1 = dict(RR_TAIL0, ks_mac=2, moddown_pass2=0, intt_pass1=1)


def _ctx(N, primes, knobs):
    env = dict(knobs, EVAH_FUSE_SMALL=0, EVAH_MODUP=1)
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


def _c60(logN, l):
    return lambda: (1 << logN, po.coeff_modulus_create(1 << logN, [60] * (l + 1)))


SHAPES = {
    "N2^12_l2": _c60(12, 2),
    "N2^12_l7": _c60(12, 7),
    "N2^12_l8": _c60(12, 8),
    "N2^12_l15": _c60(12, 15),
    "N2^13_l3": _c60(13, 3),
    "N2^15_l2": _c60(15, 2),
    "N2^16_l2": _c60(16, 2),
    "N2^12_mixed": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60, 38, 60, 40])),
    "N2^12_nontb55": lambda: (1 << 12, _nontb55(1 << 12)),
}
KINDS = ("random", "qm1", "dense_max")
CASES = [f"{s}-{k}" for s in SHAPES for k in KINDS]
CALLS = ("relinearize", "rotate", "relinearize_rescale", "triple_1", "triple_3")


def _counts(g, call):
    g.profile(True)
    g.profile_reset()
    keep = call()  # the result stays alive until the launches have run
    g.sync()
    del keep
    out = {name: n for name, (n, _) in g.profile_get().items()}
    g.profile(False)
    return out


def _same(counts, want):
    return {k: counts.get(k, 0) for k in want} == want and sum(counts.values()) == sum(want.values())


class _Case:
    """keys, operands and the oracle's words of one case: computed once, shared by the tests, never written to"""

    def __init__(self, name):
        shape, kind = name.split("-")
        self.N, self.primes = SHAPES[shape]()
        N, primes = self.N, self.primes
        k = len(primes)
        l = self.l = k - 1
        self.mac3 = "nontb" not in shape
        self.div = int(primes[-2]).bit_length()
        o = po.Oracle(N, primes)
        rng = np.random.default_rng(N + k)

        def rand(prefix, nl):
            return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))
        if kind == "random":
            self.rk, self.gk = rand((l, 2), k), rand((l, 2), k)
            self.ops = [(rand((2,), l), rand((2,), l)) for _ in range(3)]
            self.m = o.multiply(*self.ops[0])
            triples = [o.op_triple(a, b, self.rk) for a, b in self.ops]
        else:  # worst-case words: keys at q - 1; every residue (qm1) / every coefficient (dense_max) at q - 1
            self.rk = self.gk = np.stack([np.full((l, 2, N), primes[i] - 1, dtype=np.uint64) for i in range(k)], axis=2)
            if kind == "qm1":
                p = np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])
            else:
                p = np.stack([o.ntt(i, np.full(N, primes[i] - 1, dtype=np.uint64)) for i in range(l)])
            self.ops = [(np.stack([p, p]), np.stack([p, p]))] * 3
            self.m = np.stack([p, p, p])  # the key-switch target is the worst-case polynomial itself
            triples = [o.op_triple(*self.ops[0], self.rk)] * 3
        relin = o.relinearize(self.m, self.rk)
        self.want = {
            "relinearize": [relin],
            "rotate": [o.rotate(self.ops[0][0], STEP, self.gk)],
            "relinearize_rescale": [o.rescale(relin)],
            "triple_1": triples[:1],
            "triple_3": triples,
        }
        for v in self.want.values():
            for w in v:
                w.setflags(write=False)

    def calls(self, g):
        M = g.upload_ct(self.m, 2.0 ** 60)
        A = [g.upload_ct(a, 2.0 ** 30) for a, _ in self.ops]
        B = [g.upload_ct(b, 2.0 ** 30) for _, b in self.ops]
        return {
            "relinearize": lambda: [g.relinearize(M)],
            "rotate": lambda: [g.rotate(A[0], STEP)],
            "relinearize_rescale": lambda: [g.relinearize_rescale(M, self.div)],
            "triple_1": lambda: g.multiply_relinearize_rescale_many(A[:1], B[:1], self.div),
            "triple_3": lambda: g.multiply_relinearize_rescale_many(A, B, self.div),
        }

    def context(self, ks_tail):
        g = _ctx(self.N, self.primes, {"EVAH_KS_TAIL": ks_tail})
        g.upload_relin_key(self.rk)
        g.upload_galois_key(g.galois_elt_from_step(STEP), self.gk)
        return g


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        _CACHE.clear()  # (the cases of one shape and kind follow each other: one at a time stays resident)
        _CACHE[name] = _Case(name)
    return _CACHE[name]


def _check_words(c, g, which):
    calls = c.calls(g)
    for what in which:
        got = [x.download() for x in calls[what]()]
        assert len(got) == len(c.want[what]), what
        for i, (x, y) in enumerate(zip(got, c.want[what])):
            assert np.array_equal(x, y), f"{what} [{i}]: differs from the oracle"
    return calls


@pytest.mark.parametrize("name", CASES)
def test_tail_slices_leave_the_oracle_words(name):
    """EVAH_KS_TAIL=1: relinearize and the rotation store prod (no tail epilogue); relinearize + rescale and the op-triple run
    slices A and B.  A chain without the radix-2^30 kernel keeps the 128-bit kernel's launches."""
    c = _case(name)
    g = c.context(1)
    try:
        assert g.ks_tail() == (c.mac3, 0), g.ks_tail()
        # the radix-2^30 kernel multiplies with the keys' split copies: they exist exactly where it is selected — at l = 15 too
        words, split, _ = g.key_bytes_detail()
        assert split == (words if c.mac3 else 0), (words, split)
        calls = _check_words(c, g, CALLS)
        for what in ("relinearize_rescale", "triple_1", "triple_3"):
            n = _counts(g, calls[what])
            assert _same(n, RR_TAIL1 if c.mac3 else RR_TAIL0), (what, n)
        # relinearize and the rotation: the mod-up kernel and ONE key-switch launch (tables below)
        n = _counts(g, calls["relinearize"])
        assert n["ks_mac"] == 1 and n["ksdigit_pass1"] == 1 and n["ksdigit_pass2"] == 0, n
        assert _same(n, RELIN[c.mac3]), n
        n = _counts(g, calls["rotate"])
        assert n["ks_mac"] == 1 and n["ksdigit_pass1"] == 1 and n["ksdigit_pass2"] == 0, n
        assert _same(n, ROTATE[c.mac3]), n
    finally:
        g.close()


@pytest.mark.parametrize("name", CASES)
def test_stored_products_leave_the_oracle_words(name):
    """EVAH_KS_TAIL=0: the same kernel without a tail epilogue (KS_TAIL_NONE) stores prod for the three-launch tail"""
    c = _case(name)
    g = c.context(0)
    try:
        assert g.ks_tail() == (False, 0), g.ks_tail()
        calls = _check_words(c, g, ("relinearize_rescale", "triple_1", "triple_3"))
        for what in ("relinearize_rescale", "triple_1", "triple_3"):
            n = _counts(g, calls[what])
            assert _same(n, RR_TAIL0), (what, n)
    finally:
        g.close()


# one relinearize and one rotation (the same launches on the radix-2^30 and the 128-bit kernel): inverse transform of the
# target's digits, mod-up, ONE key-switch launch, the special rows' strided inverse pass and the mod-down's two passes; the
# rotation's permutation launch in front
_RELIN = dict(ZERO, intt_pass1=2, intt_pass2=1, ksdigit_pass1=1, ks_mac=1, moddown_pass1=1, moddown_pass2=1)
RELIN = {True: _RELIN, False: _RELIN}
ROTATE = {True: dict(_RELIN, elementwise=1), False: dict(_RELIN, elementwise=1)}
