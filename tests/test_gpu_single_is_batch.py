"""The single evaluator key-switch calls are their `_many` forms with one instance: same words, same handle, same launches.

For every pair (relinearize, relinearize_rescale, multiply_relinearize_rescale, multiply_rescale_relinearize,
rescale_relinearize, rescale — each against its `_many` form with n = 1) the two calls return the oracle's words, equal
info() and equal per-class launch counts (profile(True), profile_reset(), the call, sync(), profile_get(), as
test_gpu_extremes._relinearize_launches takes them).  A batched handle of B = 3 instances through relinearize and
relinearize_rescale equals, in words and in launches, the `_many` call on the three instances uploaded separately.
The contexts are the smallest at which each launch form is reached:
  N1024        [60, 60, 60]                        partial tile, two-launch form
  small        N = 4096, [60] * 4                  small-launch form, MAC3, fused special-row inverse pass
  modup        the same, EVAH_FUSE_SMALL=0         mod-up kernel
  N8192_bits30 [60, 30, 60, 60]                    no MAC3, generic butterflies
  fold_pa0     N = 4096, [60] * 4, EVAH_FOLD_PA=0  the OpRR / OpRRLast / add_tab forms
  fuse_mac0    ... EVAH_FUSE_MAC=0                 the unfused path and its fallbacks
  chain_step0  ... EVAH_CHAIN_STEP=0               the two-call rescale_relinearize fallback
and one error case: with EVAH_CHAIN_STEP=0, rescale_relinearize_many on two handles of which the second is at level 1
raises "end of modulus switching chain reached" and leaves no device memory held."""
import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po
from test_gpu_extremes import _ctx, _same

pytestmark = pytest.mark.gpu

CONTEXTS = [
    ("N1024", 1 << 10, [60, 60, 60], {}),
    ("small", 1 << 12, [60] * 4, {}),
    ("modup", 1 << 12, [60] * 4, {"EVAH_FUSE_SMALL": 0}),
    ("N8192_bits30", 1 << 13, [60, 30, 60, 60], {}),
    ("fold_pa0", 1 << 12, [60] * 4, {"EVAH_FOLD_PA": 0}),
    ("fuse_mac0", 1 << 12, [60] * 4, {"EVAH_FUSE_MAC": 0}),
    ("chain_step0", 1 << 12, [60] * 4, {"EVAH_CHAIN_STEP": 0}),
]
B = 3


def _rand(rng, primes, N, prefix, nl):
    return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))


class _Case:
    """one context with its relinearization key, B random size-3 ciphertexts and two random size-2 operands"""

    def __init__(self, N, bits, knobs):
        self.N, self.primes = N, po.coeff_modulus_create(N, bits)
        self.k = len(self.primes)
        self.l = self.k - 1
        self.div = int(self.primes[-2]).bit_length()
        self.o = po.Oracle(N, self.primes)
        self.rng = np.random.default_rng(N + len(knobs))
        self.rk = self.rand((self.l, 2), self.k)
        self.g = _ctx(N, self.primes, knobs)
        self.g.upload_relin_key(self.rk)
        self.m = [self.rand((3,), self.l) for _ in range(B)]
        self.a, self.b = self.rand((2,), self.l), self.rand((2,), self.l)
        self.relin = [self.o.relinearize(m, self.rk) for m in self.m]  # shared by the tests of the context, never written

    def rand(self, prefix, nl):
        return _rand(self.rng, self.primes, self.N, prefix, nl)

    def run(self, fn):
        """fn() -> list of handles; ([words], [info], {kernel class: launches})"""
        g = self.g
        g.profile(True)
        g.profile_reset()
        outs = fn()
        g.sync()
        prof = g.profile_get()
        g.profile(False)
        return [c.download() for c in outs], [c.info() for c in outs], {name: n for name, (n, _) in prof.items()}


@pytest.fixture(scope="module", params=CONTEXTS, ids=[c[0] for c in CONTEXTS])
def case(request):
    _, N, bits, knobs = request.param
    p = _Case(N, bits, knobs)
    yield p
    p.g.close()


def test_single_call_is_the_many_call_of_one(case):
    p, g, o, rk, div = case, case.g, case.o, case.rk, case.div
    m3 = p.m[0]
    M3 = g.upload_ct(m3, 2.0 ** 60)
    A, Bb = g.upload_ct(p.a, 2.0 ** 30), g.upload_ct(p.b, 2.0 ** 30)
    prod = o.multiply(p.a, p.b)
    pairs = [
        ("relinearize", lambda: [g.relinearize(M3)], lambda: g.relinearize_many([M3]), p.relin[0]),
        ("relinearize_rescale", lambda: [g.relinearize_rescale(M3, div)], lambda: g.relinearize_rescale_many([M3], div),
         o.rescale(p.relin[0])),
        ("multiply_relinearize_rescale", lambda: [g.multiply_relinearize_rescale(A, Bb, div)],
         lambda: g.multiply_relinearize_rescale_many([A], [Bb], div), o.rescale(o.relinearize(prod, rk))),
        ("multiply_rescale_relinearize", lambda: [g.multiply_rescale_relinearize(A, Bb, div)],
         lambda: g.multiply_rescale_relinearize_many([A], [Bb], div), o.relinearize(o.rescale(prod), rk)),
        ("rescale_relinearize", lambda: [g.rescale_relinearize(M3, div)], lambda: g.rescale_relinearize_many([M3], div),
         o.relinearize(o.rescale(m3), rk)),
        ("rescale", lambda: [g.rescale(M3, div)], lambda: g.rescale_many([M3], div), o.rescale(m3)),
    ]
    for name, single, many, want in pairs:
        w1, i1, n1 = p.run(single)
        wn, in_, nn = p.run(many)
        print(name, "single", n1, "many", nn)
        assert len(w1) == len(wn) == 1
        _same(w1[0], want, f"{name}")
        _same(wn[0], want, f"{name}_many")
        assert i1 == in_, name
        assert n1 == nn, name


def test_batched_handle_is_the_many_call_on_its_instances(case):
    p, g, o, div = case, case.g, case.o, case.div
    Bh = g.upload_ct_batch(np.stack(p.m), 2.0 ** 60)
    Ms = [g.upload_ct(m, 2.0 ** 60) for m in p.m]
    pairs = [
        ("relinearize", lambda: [g.relinearize(Bh)], lambda: g.relinearize_many(Ms), p.relin),
        ("relinearize_rescale", lambda: [g.relinearize_rescale(Bh, div)], lambda: g.relinearize_rescale_many(Ms, div),
         [o.rescale(r) for r in p.relin]),
    ]
    for name, batched, many, want in pairs:
        wb, ib, nb = p.run(batched)
        wn, in_, nn = p.run(many)
        print(name, "batched", nb, "many", nn)
        assert wb[0].shape[0] == len(wn) == B
        for b in range(B):
            _same(wb[0][b], want[b], f"{name}, batched handle, instance {b}")
            _same(wn[b], want[b], f"{name}_many [{b}]")
            assert in_[b] == ib[0], name
        assert nb == nn, name


def test_failing_two_call_fallback_holds_no_memory():
    N = 1 << 12
    primes = po.coeff_modulus_create(N, [60] * 4)
    l = len(primes) - 1
    rng = np.random.default_rng(11)
    g = _ctx(N, primes, {"EVAH_CHAIN_STEP": 0})
    try:
        g.upload_relin_key(_rand(rng, primes, N, (l, 2), len(primes)))
        first, second = g.upload_ct(_rand(rng, primes, N, (3,), l), 2.0 ** 60), g.upload_ct(_rand(rng, primes, N, (3,), 1), 2.0 ** 60)
        g.sync()
        before = g.mem_info()[0]
        with pytest.raises(backend.EvaHipError, match="end of modulus switching chain reached"):
            g.rescale_relinearize_many([first, second], 60)
        g.sync()
        after = g.mem_info()[0]
        print("device bytes in use before", before, "after", after)
        assert after <= before
    finally:
        g.close()
