"""The key switch's mod-up at throughput size (ntt_modup_kernel, EVAH_MODUP): one workgroup per digit tile runs the
digit's strided inverse pass once and its conversion + forward strided pass under every output prime.  It must leave
the same lazy intermediates as the two-launch form, so every result is the oracle's words AND, word for word, what a
context with EVAH_MODUP=0 returns.  Shapes: the headline's (N = 2^16, l = 10, 1 / 32 / 64 fused op-triples), stored
products through relinearize / relinearize + rescale, chains with primes not of the top-bit shape (compare-and-subtract
butterflies; with and without the radix-2^30 inner product), more than 16 digits, N = 2^12 and 2^15, a batched handle.  Small shapes are
pushed past the fused small-launch form with EVAH_FUSE_SMALL=0 so that they take the mod-up kernel too; among them the
two ends of the kernel's P dispatch: N = 2^11 (P = 6 with ONE column tile per digit, so the digit index is the whole of
blockIdx.x) and N = 2^17 (P = 9, at l = 2 to keep the oracle quick).  Every shape of test_other_shapes also counts
launches (_Pair.ran_on_modup): the EVAH_MODUP=1 context must have run the digits' strided inverse pass inside the
ksdigit_pass1 launch, or the comparison covers nothing.  The other callers of the key switch, the launch counts
themselves and the gate are in test_gpu_modup_forms.py; worst-case words on this kernel in test_gpu_extremes.py."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _ctx(N, primes, knobs):
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update({k: str(v) for k, v in knobs.items()})
    try:
        return backend.Context(N, primes)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Pair:
    """The same keys and operands on a context with the mod-up kernel and one without."""

    def __init__(self, N, primes, extra=None, seed=0):
        self.N, self.primes = N, primes
        self.k = len(self.primes)
        self.l = self.k - 1
        self.div = int(primes[-2]).bit_length()
        self.o = po.Oracle(N, self.primes)
        self.rng = np.random.default_rng(seed)
        self.rk = self.rand((self.l, 2), self.k)
        extra = extra or {}
        self.ctx = {m: _ctx(N, self.primes, dict(extra, EVAH_MODUP=m)) for m in (1, 0)}
        for g in self.ctx.values():
            g.upload_relin_key(self.rk)

    def rand(self, prefix, nl):
        return np.stack([self.rng.integers(0, self.primes[i], size=prefix + (self.N,), dtype=np.uint64) for i in range(nl)],
                        axis=len(prefix))

    def both(self, fn):
        """fn(context) -> list of arrays; the two settings' words, asserted equal, from the EVAH_MODUP=1 context"""
        got = {m: fn(g) for m, g in self.ctx.items()}
        for x, y in zip(got[1], got[0]):
            assert np.array_equal(x, y), "EVAH_MODUP=1 and EVAH_MODUP=0 differ"
        return got[1]

    def launches(self, fn):
        """{EVAH_MODUP setting: {kernel class: launches}} of fn(context)"""
        out = {}
        for m, g in self.ctx.items():
            g.profile(True)
            g.profile_reset()
            keep = fn(g)  # results stay alive until the launches have run
            g.sync()
            del keep
            out[m] = {name: n for name, (n, _) in g.profile_get().items()}
            g.profile(False)
        return out

    def ran_on_modup(self, fn, calls=1):
        """fn(context) holds `calls` key switches: under EVAH_MODUP=1 each one's stand-alone strided inverse pass of the
        digits (an intt_pass2 launch) is gone, into the ksdigit_pass1 launch it had anyway; no other count moves"""
        n = self.launches(fn)
        assert n[0]["intt_pass2"] >= calls and n[0]["ksdigit_pass1"] >= calls, n
        assert n[1] == dict(n[0], intt_pass2=n[0]["intt_pass2"] - calls), n

    def close(self):
        for g in self.ctx.values():
            g.close()


def _triples(p, n, distinct=3):
    """n fused op-triples over `distinct` operand pairs (cycled), each against the oracle"""
    ops = [(p.rand((2,), p.l), p.rand((2,), p.l)) for _ in range(distinct)]
    want = [p.o.op_triple(a, b, p.rk) for a, b in ops]

    def run(g):
        up = [(g.upload_ct(a, 2.0 ** 30), g.upload_ct(b, 2.0 ** 30)) for a, b in ops]
        return [c.download() for c in g.multiply_relinearize_rescale_many([up[i % distinct][0] for i in range(n)],
                                                                          [up[i % distinct][1] for i in range(n)], p.div)]
    for i, got in enumerate(p.both(run)):
        assert np.array_equal(got, want[i % distinct]), f"triple {i}"


def _ntt_prime_below(bound, N):
    q = bound - (bound % (2 * N)) + 1
    while q >= bound or not po.lib.evo_is_prime(q):
        q -= 2 * N
    return q


def _stored(p):
    """relinearize / relinearize + rescale of a stored product: single, many, a batched handle"""
    a, b = p.rand((2,), p.l), p.rand((2,), p.l)
    m = p.o.multiply(a, b)
    relin = p.o.relinearize(m, p.rk)
    triple = p.o.op_triple(a, b, p.rk)

    def run(g):
        M = g.upload_ct(m, 2.0 ** 60)
        MB = g.upload_ct_batch(np.stack([m, m, m]), 2.0 ** 60)
        out = [g.relinearize(M).download(), g.relinearize_rescale(M, p.div).download()]
        out += [c.download() for c in g.relinearize_many([M, M])]
        out += [c.download() for c in g.relinearize_rescale_many([M, M], p.div)]
        out += list(g.relinearize(MB).download()) + list(g.relinearize_rescale(MB, p.div).download())
        return out
    got = p.both(run)
    for x in got[0:1] + got[2:4] + got[6:9]:
        assert np.array_equal(x, relin), "relinearize"
    for x in got[1:2] + got[4:6] + got[9:12]:
        assert np.array_equal(x, triple), "relinearize + rescale"


@pytest.mark.parametrize("n", [1, 32, 64])
def test_headline_triples(n):
    """N = 2^16, l = 10: every one of these key switches is throughput-sized"""
    p = _Pair(1 << 16, po.coeff_modulus_create(1 << 16, [60] * 11), seed=n)
    try:
        _triples(p, n)
    finally:
        p.close()


def test_headline_stored_products():
    p = _Pair(1 << 16, po.coeff_modulus_create(1 << 16, [60] * 11), seed=5)
    try:
        _stored(p)
    finally:
        p.close()


def _shapes():
    c60 = po.coeff_modulus_create(1 << 13, [60] * 5)
    nontb = _ntt_prime_below((1 << 55) - (1 << 40), 1 << 13)  # 2^55 - c with c >= 2^32, above 2^54: no top-bit shape
    return [
        ("N4096", 1 << 12, po.coeff_modulus_create(1 << 12, [60] * 11), {}, 4),       # P = 6
        ("N32768", 1 << 15, po.coeff_modulus_create(1 << 15, [60] * 11), {}, 4),      # P = 8 over 7-bit contiguous sub-transforms
        ("l17", 1 << 14, po.coeff_modulus_create(1 << 14, [60] * 18), {}, 4),         # more than 16 digits (128-bit inner products)
        # compare-and-subtract butterflies under a 30-bit prime (the radix-2^30 inner products still apply) / under a
        # 55-bit prime of no top-bit shape (128-bit inner products)
        ("bits30", 1 << 13, po.coeff_modulus_create(1 << 13, [60, 30, 60, 60, 60]), {}, 4),
        ("nontb55", 1 << 13, [c60[0], nontb, c60[1], c60[2], c60[4]], {}, 4),
        # the ends of the P dispatch: P = 6 with one column tile per digit (log_tiles = 0) / P = 9
        ("N2048", 1 << 11, po.coeff_modulus_create(1 << 11, [50, 50, 50, 51]), {}, 2),
        ("N131072", 1 << 17, po.coeff_modulus_create(1 << 17, [60] * 3), {}, 2),
    ]


SHAPES = _shapes()


@pytest.mark.parametrize("name,N,primes,knobs,triples", SHAPES, ids=[s[0] for s in SHAPES])
def test_other_shapes(name, N, primes, knobs, triples):
    """small shapes pushed past the fused small-launch form (EVAH_FUSE_SMALL=0) so that they take the mod-up kernel"""
    p = _Pair(N, primes, extra=dict(knobs, EVAH_FUSE_SMALL=0), seed=N + len(primes))
    try:
        _triples(p, triples, distinct=2)
        _stored(p)
        m = p.rand((3,), p.l)
        p.ran_on_modup(lambda g: g.relinearize(g.upload_ct(m, 2.0 ** 60)))
    finally:
        p.close()
