"""The mod-up kernel (ntt_modup_kernel, EVAH_MODUP) through every caller of the key switch, and proof that it is the path
that ran.  test_gpu_modup.py reaches it through the relinearize family and multiply_relinearize_rescale_many; here:
  launch accounting   one relinearize of a stored size-3 ciphertext at (N = 4096, l = 4, EVAH_FUSE_SMALL=0) is seven
                      launches with the kernel and eight without (the digits' strided inverse pass, an intt_pass2 launch,
                      moves into the ksdigit_pass1 launch); with EVAH_FUSE_SMALL at its default both settings take the
                      small-launch form, five launches — which pins the gate;
  every other caller  rotate (switch_key), the unhoisted rotation set (rotate_many, rotate_pairs with EVAH_HOIST=0,
                      rotate_weighted_sums with EVAH_WIN_FUSE=0: targets at stride 2 l N inside the permuted pairs), the
                      launch set multiply_rescale_relinearize(_many) and rescale_relinearize(_many) take with
                      EVAH_CHAIN_STEP=0 (targets at stride 3 (l - 1) N inside the rescaled polynomials), the same on two
                      streams (EVAH_SIDE_STREAM=1: a limb-contiguous target and no folded addends), and the fused
                      multiply on a batched handle.
Random words at (N = 4096, 60-bit primes) and at N = 8192 with a 30-bit prime in the chain, EVAH_FUSE_SMALL=0 throughout.
Every result is the oracle's words and, word for word, what the EVAH_MODUP=0 context returns; each knob set also counts
launches once (_Pair.ran_on_modup), so a caller that stopped reaching the kernel would fail here."""
import numpy as np
import pytest

from oracle import pyoracle as po
from test_gpu_modup import _Pair

pytestmark = pytest.mark.gpu

CLASSES = ("elementwise", "intt_pass1", "intt_pass2", "ksdigit_pass1", "ksdigit_pass2", "ks_mac", "moddown_pass1",
           "moddown_pass2", "ntt_pass1", "ntt_pass2")


def _counts(**n):
    return {c: n.get(c, 0) for c in CLASSES}


def test_the_mod_up_kernel_is_the_one_that_runs():
    """switch_key_products + the mod-down of switch_key, one key switch too large for the small-launch form:
      EVAH_MODUP=0  contiguous + strided inverse pass of the digits, OpKsDigit strided pass, key-switch kernel; the
                    special rows' inverse transform (two passes), the mod-down's two forward passes: 8 launches
      EVAH_MODUP=1  the digits' strided inverse pass runs inside the ksdigit_pass1 launch: 7
    and with EVAH_FUSE_SMALL at its default the shape is small whatever EVAH_MODUP says: contiguous inverse pass,
    ntt_inv_fwd_kernel (ksdigit_pass1), the key-switch kernel with the special rows' first inverse pass inside it,
    ntt_inv_fwd_kernel of the mod-down (moddown_pass1), its second pass."""
    N, primes = 4096, po.coeff_modulus_create(4096, [60] * 5)
    relin = lambda m: (lambda g: g.relinearize(g.upload_ct(m, 2.0 ** 60)))
    p = _Pair(N, primes, extra={"EVAH_FUSE_SMALL": 0}, seed=1)
    try:
        m = p.rand((3,), p.l)
        n = p.launches(relin(m))
        assert n[0] == _counts(intt_pass1=2, intt_pass2=2, ksdigit_pass1=1, ks_mac=1, moddown_pass1=1, moddown_pass2=1), n[0]
        assert n[1] == _counts(intt_pass1=2, intt_pass2=1, ksdigit_pass1=1, ks_mac=1, moddown_pass1=1, moddown_pass2=1), n[1]
        want = p.o.relinearize(m, p.rk)
        assert np.array_equal(p.both(lambda g: [relin(m)(g).download()])[0], want)
    finally:
        p.close()
    p = _Pair(N, primes, seed=1)
    try:
        n = p.launches(relin(m))
        assert n[1] == n[0] == _counts(intt_pass1=1, ksdigit_pass1=1, ks_mac=1, moddown_pass1=1, moddown_pass2=1), n
    finally:
        p.close()


STEPS = [1, -3]


class _Callers(_Pair):
    """_Pair with Galois keys for STEPS and two random size-2 operands"""

    def __init__(self, N, primes, knobs, seed):
        super().__init__(N, primes, extra=dict(knobs, EVAH_FUSE_SMALL=0), seed=seed)
        self.gk = {st: self.rand((self.l, 2), self.k) for st in STEPS}
        for g in self.ctx.values():
            for st in STEPS:
                g.upload_galois_key(g.galois_elt_from_step(st), self.gk[st])
        self.a, self.b = self.rand((2,), self.l), self.rand((2,), self.l)

    def rot(self, a, st):
        return self.o.rotate(a, st, self.gk[st])

    def check(self, fn, want, what):
        got = self.both(fn)
        assert len(got) == len(want), what
        for i, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), f"{what} [{i}]"


def _default(p):
    a, b = p.a, p.b
    up = lambda g, x: g.upload_ct(x, 2.0 ** 30)
    p.check(lambda g: [g.rotate(up(g, a), st).download() for st in STEPS], [p.rot(a, st) for st in STEPS], "rotate")
    p.check(lambda g: [c.download() for c in g.rotate_many(up(g, a), STEPS)], [p.rot(a, st) for st in STEPS], "rotate_many")
    xs, ys = [a, b, p.rand((2,), p.l)], [b, b, a]
    p.check(lambda g: list(g.multiply_relinearize_rescale(g.upload_ct_batch(np.stack(xs), 2.0 ** 30),
                                                          g.upload_ct_batch(np.stack(ys), 2.0 ** 30), p.div).download()),
            [p.o.op_triple(x, y, p.rk) for x, y in zip(xs, ys)], "multiply_relinearize_rescale, batched handle")
    p.ran_on_modup(lambda g: g.rotate(up(g, a), 1))


def _unhoisted(p):
    a, b = p.a, p.b
    up = lambda g, x: g.upload_ct(x, 2.0 ** 30)
    p.check(lambda g: [c.download() for c in g.rotate_many(up(g, a), STEPS)], [p.rot(a, st) for st in STEPS], "rotate_many")
    if hasattr(next(iter(p.ctx.values())), "rotate_pairs"):
        def pairs(g):
            A, B = up(g, a), up(g, b)
            return [c.download() for c in g.rotate_pairs([A, A, B], [1, -3, 1])]
        p.check(pairs, [p.rot(a, 1), p.rot(a, -3), p.rot(b, 1)], "rotate_pairs")
    p.ran_on_modup(lambda g: g.rotate_many(up(g, a), STEPS))


def _window(p):
    a = p.a
    wts = [p.rand((), p.l) for _ in range(3)]
    want = None
    for r, w in zip([a] + [p.rot(a, st) for st in STEPS], wts):
        t = p.o.multiply_plain(r, w)
        want = t if want is None else p.o.add(want, t)

    def run(g):
        A = g.upload_ct(a, 2.0 ** 30)
        W = [g.upload_pt(w, 2.0 ** 10) for w in wts]
        return g.rotate_weighted_sums([([(A, st) for st in [0] + STEPS], [W])])
    p.check(lambda g: [c.download() for c in run(g)], [want], "rotate_weighted_sums")
    p.ran_on_modup(run)


def _chain(p, many=True):
    a, b = p.a, p.b
    o, rk = p.o, p.rk
    up = lambda g, x: g.upload_ct(x, 2.0 ** 30)
    step = lambda x, y: o.relinearize(o.rescale(o.multiply(x, y)), rk)
    p.check(lambda g: [g.multiply_rescale_relinearize(up(g, a), up(g, b), p.div).download()], [step(a, b)],
            "multiply_rescale_relinearize")
    p.ran_on_modup(lambda g: g.multiply_rescale_relinearize(up(g, a), up(g, b), p.div))
    if not many:
        return
    p.check(lambda g: [c.download() for c in g.multiply_rescale_relinearize_many([up(g, a), up(g, b)], [up(g, b), up(g, b)], p.div)],
            [step(a, b), step(b, b)], "multiply_rescale_relinearize_many")
    m = [o.multiply(a, b), o.multiply(a, a)]
    want = [o.relinearize(o.rescale(x), rk) for x in m]
    up3 = lambda g, x: g.upload_ct(x, 2.0 ** 60)
    p.check(lambda g: [g.rescale_relinearize(up3(g, m[0]), p.div).download()], want[:1], "rescale_relinearize")
    p.check(lambda g: [c.download() for c in g.rescale_relinearize_many([up3(g, m[0]), up3(g, m[1])], p.div)], want,
            "rescale_relinearize_many")
    p.check(lambda g: list(g.multiply_rescale_relinearize(g.upload_ct_batch(np.stack([a, b]), 2.0 ** 30),
                                                          g.upload_ct_batch(np.stack([b, b]), 2.0 ** 30), p.div).download()),
            [step(a, b), step(b, b)], "multiply_rescale_relinearize, batched handle")


KNOB_SETS = [
    ("default", {}, _default),
    ("hoist0", {"EVAH_HOIST": 0}, _unhoisted),
    ("win_fuse0", {"EVAH_WIN_FUSE": 0}, _window),
    ("chain_step0", {"EVAH_CHAIN_STEP": 0}, _chain),
    ("side_stream", {"EVAH_CHAIN_STEP": 0, "EVAH_SIDE_STREAM": 1}, lambda p: _chain(p, many=False)),
]
CHAINS = [("N4096_60x5", 1 << 12, [60] * 5), ("N8192_bits30", 1 << 13, [60, 30, 60, 60, 60])]


@pytest.mark.parametrize("shape,N,bits", CHAINS, ids=[c[0] for c in CHAINS])
@pytest.mark.parametrize("name,knobs,body", KNOB_SETS, ids=[k[0] for k in KNOB_SETS])
def test_callers_of_the_key_switch(shape, N, bits, name, knobs, body):
    p = _Callers(N, po.coeff_modulus_create(N, bits), knobs, seed=N + len(name))
    try:
        body(p)
    finally:
        p.close()
