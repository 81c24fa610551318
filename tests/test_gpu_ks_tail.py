"""The relinearize + rescale tail with its two contiguous passes inside the key-switch kernel (EVAH_KS_TAIL=1: mod-up, key-switch
slice A, ntt_tail_kernel, key-switch slice B — five launches, the key-switch products never stored) leaves the words of the
six launches (EVAH_KS_TAIL=0) and of the oracle.

The path runs where the key switch takes the mod-up kernel, so EVAH_FUSE_SMALL=0 pushes the small shapes here past the
small-launch form, as in test_gpu_tail_fused.py.  Each case gives the same keys and operands to two contexts that differ in
EVAH_KS_TAIL only and compares, word for word: the fused op-triple (multiply_relinearize_rescale_many with 1, 3 and 64
products — at N = 2^12 the 64 are the KS_BATCH_MAX edge of the (tile, instance) placement in blockIdx.x — and on a batched
handle) and relinearize_rescale of a stored product (single, _many with 3 handles, a batched handle).  Launch counts of one
relinearize_rescale and one op-triple call prove which path ran.
Cases:
  N = 2^12 (passes 6, 6: four sub-transforms per key-switch tile) and N = 2^13 (7, 6: the odd split);
  four 60-bit primes (l = 3: two data rows in slice B) and three (l = 2: slice B is one row, one output row in the tail kernel);
  N = 2^12 with 60, 38, 60-bit data primes and a 40-bit special prime: all top-bit, but the tail kernel is not lazy-only;
  operands: uniform random words; every residue at q - 1 (qm1) and every coefficient of limb J at q_J - 1 (dense_max), with
      keys at q - 1 — the worst-case words of test_gpu_extremes.py;
  the nontb55 chain of test_gpu_extremes.py (a 55-bit prime of no top-bit shape: 128-bit inner products) is not eligible: the
      query says so and the launches are the six-launch path's, knob or not.
Without the knob the path is taken by size (slice A must fill the chip): the shapes here keep the six launches then, and
EVAH_KS_TAIL_MIN_WGS moves the threshold."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

# launches per kernel class of one relinearize + rescale launch set at the mod-up kernel's size: the three-launch tail ...
OLD = {"elementwise": 0, "intt_pass1": 2, "intt_pass2": 0, "ksdigit_pass1": 1, "ksdigit_pass2": 0, "ks_mac": 1,
       "moddown_pass1": 1, "moddown_pass2": 1, "ntt_pass1": 0, "ntt_pass2": 0}
# ... and with the tail's contiguous passes inside the two key-switch slices
NEW = dict(OLD, ks_mac=2, moddown_pass2=0, intt_pass1=1)


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


SHAPES = {
    "N4096_60x4": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60] * 4)),
    "N8192_60x4": lambda: (1 << 13, po.coeff_modulus_create(1 << 13, [60] * 4)),
    "N4096_60x3": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60] * 3)),
    "N8192_60x3": lambda: (1 << 13, po.coeff_modulus_create(1 << 13, [60] * 3)),
    "N4096_mixed": lambda: (1 << 12, po.coeff_modulus_create(1 << 12, [60, 38, 60, 40])),
    "N4096_nontb55": lambda: (1 << 12, _nontb55(1 << 12)),
}
KINDS = ("random", "qm1", "dense_max")
ELIGIBLE = [f"{s}-{k}" for s in SHAPES if "nontb" not in s for k in KINDS]


class _Case:
    """keys, operands, the oracle's words, and the EVAH_KS_TAIL=0 context's words and launch counts of one case"""

    def __init__(self, name):
        shape, kind = name.split("-")
        self.N, self.primes = SHAPES[shape]()
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
        # in the order of run(): op-triple of 1, of 3, of 64 (product i = operands i mod 3), batched (instances 0 and 1);
        # relinearize_rescale single, x3, batched x2
        self.want = [triples[0]] + triples + [triples[i % 3] for i in range(64)] + triples[:2] + [rr] * 6
        g = _ctx(N, primes, {"EVAH_KS_TAIL": 0})
        try:
            assert g.ks_tail() == (False, 0)
            self.ref = self.run(g)
            self.ref_launches = self.launches(g)
        finally:
            g.close()
        assert len(self.ref) == len(self.want)
        for i, (got, want) in enumerate(zip(self.ref, self.want)):
            assert np.array_equal(got, want), f"result {i}: EVAH_KS_TAIL=0 differs from the oracle"

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
        out += [c.download() for c in g.multiply_relinearize_rescale_many([A[i % 3] for i in range(64)], [B[i % 3] for i in range(64)], self.div)]
        AB = [g.upload_ct_batch(np.stack([self.ops[0][x], self.ops[1][x]]), 2.0 ** 30) for x in (0, 1)]
        out += list(g.multiply_relinearize_rescale(AB[0], AB[1], self.div).download())
        out.append(g.relinearize_rescale(M, self.div).download())
        out += [c.download() for c in g.relinearize_rescale_many([M, M, M], self.div)]
        M2 = g.upload_ct_batch(np.stack([self.m, self.m]), 2.0 ** 60)
        out += list(g.relinearize_rescale(M2, self.div).download())
        return out

    def launches(self, g, products=3):
        """{kernel class: launches} of one relinearize_rescale of the stored product and of one op-triple call"""
        up, M = self._upload(g)
        counts = []
        for call in (lambda: g.relinearize_rescale(M, self.div),
                     lambda: g.multiply_relinearize_rescale_many([up[i % 3][0] for i in range(products)],
                                                                 [up[i % 3][1] for i in range(products)], self.div)):
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


def _same(counts, want):
    return {k: counts.get(k, 0) for k in want} == want and sum(counts.values()) == sum(want.values())


@pytest.mark.parametrize("name", ELIGIBLE)
def test_key_switch_tail_leaves_the_same_words(name):
    c = _case(name)
    for n in c.ref_launches:  # the knob off: the launches before this path existed
        assert _same(n, OLD), n
    g = _ctx(c.N, c.primes, {"EVAH_KS_TAIL": 1})
    try:
        assert g.ks_tail() == (True, 0)
        got = c.run(g)
        assert len(got) == len(c.ref)
        for i, (x, ref, want) in enumerate(zip(got, c.ref, c.want)):
            assert np.array_equal(x, ref), f"result {i}: EVAH_KS_TAIL=1 and EVAH_KS_TAIL=0 differ"
            assert np.array_equal(x, want), f"result {i}: differs from the oracle"
        for n in c.launches(g):
            assert n["ks_mac"] == 2 and n["moddown_pass1"] == 1 and n["moddown_pass2"] == 0, n
            assert n["intt_pass1"] == 1 and n["intt_pass2"] == 0, n
            assert _same(n, NEW), n  # no other count moves
    finally:
        g.close()


@pytest.mark.parametrize("kind", ["random", "qm1"])
def test_a_chain_without_the_radix_2_30_key_switch_keeps_its_launches(kind):
    c = _case(f"N4096_nontb55-{kind}")  # (its EVAH_KS_TAIL=0 words are checked against the oracle there)
    g = _ctx(c.N, c.primes, {"EVAH_KS_TAIL": 1})
    try:
        assert g.ks_tail() == (False, 0)
        for i, (x, want) in enumerate(zip(c.run(g), c.want)):
            assert np.array_equal(x, want), f"result {i}: differs from the oracle"
        for n, ref in zip(c.launches(g), c.ref_launches):
            assert _same(n, OLD) and n == ref, (n, ref)
    finally:
        g.close()


def test_without_the_knob_the_path_is_taken_by_size():
    """unset: slice A's 2 n N / 256 workgroups must reach EVAH_KS_TAIL_MIN_WGS (4096 by default)"""
    c = _case("N4096_60x4-random")
    g = _ctx(c.N, c.primes, {})
    try:
        assert g.ks_tail() == (True, 4096)
        for n in c.launches(g):  # 32 and 96 workgroups
            assert _same(n, OLD), n
    finally:
        g.close()
    g = _ctx(c.N, c.primes, {"EVAH_KS_TAIL_MIN_WGS": 96})
    try:
        assert g.ks_tail() == (True, 96)
        one, three = c.launches(g)
        assert _same(one, OLD) and _same(three, NEW), (one, three)
        up, _ = c._upload(g)
        got = [x.download() for x in g.multiply_relinearize_rescale_many([u[0] for u in up], [u[1] for u in up], c.div)]
        for i, (x, want) in enumerate(zip(got, c.want[1:4])):
            assert np.array_equal(x, want), f"product {i}: differs from the oracle"
    finally:
        g.close()
