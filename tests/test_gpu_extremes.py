"""Worst-case words through every key-switch form and the transforms, against the oracle's words.

The other parity tests draw ciphertext and key words uniformly from [0, q), far from the bounds the lazy reductions rest
on (MAC3's fold every 7 digits and its l <= 15 gate, the 128-bit path's fold every 15, the unreduced rows of primes below
2^54, the top-bit shape).  Here the key words are q - 1, and the key-switch digits are near their maximum on every prime:
  delta  each c1 / target limb is the constant x = min(primes) - 1 in NTT form (x * delta in coefficient form), so every
         digit of every limb is x, and the transforms see zero y inputs, which push their lazy values up;
  dense  every coefficient is x (no zero coefficients: the hoisted rotations stay on their MAC kernel);
  qm1    q - 1 in every word;
  dense_max  limb J has every COEFFICIENT at q_J - 1, so every digit sits at its own prime's maximum (x above is the
         smallest prime's, which in a mixed chain leaves the larger primes' digits far below theirs).
At N = 4096 a single key switch of l <= 31 takes the fused small-launch form, so the cases above hardly reach the mod-up
kernel of throughput-sized key switches (ntt_modup_kernel).  test_key_switch_forms_on_the_mod_up_kernel and
test_other_prime_shapes_on_the_mod_up_kernel run the same words with EVAH_FUSE_SMALL=0 (l = 1, 7, 8, 15, 16, 17; the chains
with primes of no top-bit shape), and check by launch counts that the kernel is what ran.
test_digit_conversion_at_the_lazy_flag_boundary has primes on both sides of the digit conversion's rule "q_J <= 8 q_kappa:
the digit enters the forward rounds unreduced" by the narrowest margin there is (BOUNDARY below), in both launch forms.
Rounding ties (coefficients (q_last +- 1) / 2 of the dropped limb) go through rescale, the fused forms and the chain step."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu


def _ctx(N, primes, knobs):
    env = dict({"EVAH_HOIST_MIN_TILES": 0}, **knobs)
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


def _ntt_prime_above(bound, N):
    """the smallest prime q > bound with q = 1 (mod 2N)"""
    q = bound - (bound % (2 * N)) + 1
    while q <= bound or not po.lib.evo_is_prime(q):
        q += 2 * N
    return q


def _forms(o, primes, nl, N):
    """(name, poly of nl limbs in NTT form) for the four worst-case shapes"""
    x = min(primes) - 1
    delta = np.stack([np.full(N, x % primes[i], dtype=np.uint64) for i in range(nl)])
    dense = np.stack([o.ntt(i, np.full(N, x % primes[i], dtype=np.uint64)) for i in range(nl)])
    qm1 = np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(nl)])
    dense_max = np.stack([o.ntt(i, np.full(N, primes[i] - 1, dtype=np.uint64)) for i in range(nl)])
    return [("delta", delta), ("dense", dense), ("qm1", qm1), ("dense_max", dense_max)]


def _keys(primes, l, N, rng, kind):
    k = len(primes)
    qm1 = np.stack([np.full((l, 2, N), primes[i] - 1, dtype=np.uint64) for i in range(k)], axis=2)
    if kind == "qm1":
        return qm1
    mask = rng.integers(0, 2, size=qm1.shape).astype(bool)  # q - 1 mixed with zeros
    return np.where(mask, qm1, 0).astype(np.uint64)


def _ties(o, primes, nl, N):
    """a limb set whose last limb has the coefficients 0, (q_last - 1) / 2, (q_last + 1) / 2, q_last - 1 (repeated), the
    other limbs the same integers reduced: rescale's and the mod-down's rounding sits exactly on its ties"""
    ql = primes[nl - 1]
    pat = np.array([0, (ql - 1) // 2, (ql + 1) // 2, ql - 1], dtype=object)
    coeff = np.resize(pat, N)
    return np.stack([o.ntt(i, (coeff % primes[i]).astype(np.uint64)) for i in range(nl)])


# one relinearize of a stored size-3 ciphertext when its key switch runs on ntt_modup_kernel (switch_key_products +
# switch_key's mod-down, nothing in the small-launch form): the digits' strided inverse pass is inside the ksdigit_pass1
# launch, so the only intt_pass2 launch is the special rows'.  The two-launch form (EVAH_MODUP=0) has two, the small-launch
# form none (test_gpu_modup_forms.py compares the three)
MODUP_LAUNCHES = {"elementwise": 0, "intt_pass1": 2, "intt_pass2": 1, "ksdigit_pass1": 1, "ksdigit_pass2": 0, "ks_mac": 1,
                  "moddown_pass1": 1, "moddown_pass2": 1, "ntt_pass1": 0, "ntt_pass2": 0}


def _relinearize_launches(g, A3):
    g.profile(True)
    g.profile_reset()
    out = g.relinearize(A3)
    g.sync()
    prof = g.profile_get()
    g.profile(False)
    del out
    return {name: n for name, (n, _) in prof.items()}


def _same(got, want, what=""):
    """np.array_equal(got, want), and where it fails: how many words differ and the first one, as (poly, limb, coefficient)"""
    if np.array_equal(got, want):
        return
    if got.shape != want.shape:
        raise AssertionError(f"{what}: shape {got.shape}, expected {want.shape}")
    bad = np.argwhere(got != want)
    at = tuple(int(i) for i in bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {want.size} words differ, first at (poly, limb, coefficient) = {at}: "
                         f"got {int(got[at]):#x}, expected {int(want[at]):#x}")


def _check_key_switches(g, o, primes, rng, key_kind, forms=None, launches=None):
    """launches: the launch counts one relinearize must show (None: not checked)"""
    N, k = o.N, len(primes)
    l = k - 1
    rk = _keys(primes, l, N, rng, key_kind)
    g.upload_relin_key(rk)
    steps = [1, -3]
    gks = {}
    for st in steps:
        gks[st] = _keys(primes, l, N, rng, key_kind)
        g.upload_galois_key(g.galois_elt_from_step(st), gks[st])
    F = _forms(o, primes, l, N) if forms is None else forms
    div = int(primes[l - 1]).bit_length()
    for name, p in F:
        # size-3 ciphertext whose c2 (the key-switch target) is the worst-case poly; relinearize and its fused forms
        a3 = np.stack([p, p, p])
        A3 = g.upload_ct(a3, 2.0 ** 20)
        want = o.relinearize(a3, rk)
        _same(g.relinearize(A3).download(), want, f"relinearize {name} l={l}")
        if launches is not None and name == F[0][0]:
            assert _relinearize_launches(g, A3) == launches
        if l >= 2:
            _same(g.relinearize_rescale(A3, div).download(), o.rescale(want), f"relinearize_rescale {name}")
            for got in g.relinearize_rescale_many([A3, A3], div):
                _same(got.download(), o.rescale(want), f"relinearize_rescale_many {name}")
            _same(g.rescale_relinearize(A3, div).download(), o.relinearize(o.rescale(a3), rk), f"rescale_relinearize {name}")
            for got in g.rescale_relinearize_many([A3, A3], div):
                _same(got.download(), o.relinearize(o.rescale(a3), rk))
            B3 = g.upload_ct_batch(np.stack([a3, a3]), 2.0 ** 20)
            got = g.relinearize_rescale(B3, div).download()
            for b in range(2):
                _same(got[b], o.rescale(want), f"batched {name} instance {b}")
        # rotations of a size-2 ciphertext whose c1 is the poly: one, a hoisted set, a window of weighted sums
        a2 = np.stack([p, p])
        A2 = g.upload_ct(a2, 2.0 ** 20)
        for st in steps:
            _same(g.rotate(A2, st).download(), o.rotate(a2, st, gks[st]), f"rotate {st} {name} l={l}")
        for st, got in zip(steps, g.rotate_many(A2, steps)):
            _same(got.download(), o.rotate(a2, st, gks[st]), f"rotate_many {st} {name} l={l}")
        rot = [a2] + [o.rotate(a2, st, gks[st]) for st in steps]
        qm1 = np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])
        for wname, wts in (("uniform", [qm1] * 3), ("general", [qm1, p, qm1])):
            W = [g.upload_pt(w, 2.0 ** 10) for w in wts]
            acc = None
            for r, w in zip(rot, wts):
                t = o.multiply_plain(r, w)
                acc = t if acc is None else o.add(acc, t)
            got = g.rotate_weighted_sums([([(A2, st) for st in [0] + steps], [W])])[0]
            _same(got.download(), acc, f"rotate_weighted_sums {wname} {name} l={l}")
        # products: size 3, the op triple and the chain step (multiply -> rescale -> relinearize), single and many
        m = o.multiply(a2, a2)
        _same(g.multiply(A2, A2).download(), m, f"multiply {name}")
        if l >= 2:
            triple = o.rescale(o.relinearize(m, rk))
            _same(g.multiply_relinearize_rescale(A2, A2, div).download(), triple, f"mrr {name} l={l}")
            for got in g.multiply_relinearize_rescale_many([A2, A2], [A2, A2], div):
                _same(got.download(), triple)
            chain = o.relinearize(o.rescale(m), rk)
            _same(g.multiply_rescale_relinearize(A2, A2, div).download(), chain, f"chain step {name} l={l}")
            for got in g.multiply_rescale_relinearize_many([A2, A2], [A2, A2], div):
                _same(got.download(), chain)
            AB = g.upload_ct_batch(np.stack([a2, a2]), 2.0 ** 20)
            got = g.multiply_relinearize_rescale(AB, AB, div).download()
            for b in range(2):
                _same(got[b], triple, f"batched mrr {name} instance {b}")


# (N, primes, knobs): 60-bit CoeffModulus::Create chains on both sides of MAC3's folds (l = 7 | 8, 14 | 15) and its
# gate (15 | 16), and of the 128-bit path's folds (15 | 16 | 17, 30 | 31); MAC3 at its default and switched off
def _chains():
    out = []
    for l in (1, 7, 8, 14, 15, 16, 17, 30, 31):
        for mac3 in ((None, 0) if l <= 15 else (None,)):
            out.append((f"N4096_60x{l + 1}" + ("_mac3off" if mac3 == 0 else ""), 4096, [60] * (l + 1),
                        {} if mac3 is None else {"EVAH_MAC3": 0}))
    return out


CHAINS = _chains()


@pytest.mark.parametrize("name,N,bits,knobs", CHAINS, ids=[c[0] for c in CHAINS])
def test_key_switch_forms_on_worst_case_words(name, N, bits, knobs):
    primes = po.coeff_modulus_create(N, bits)
    o = po.Oracle(N, primes)
    g = _ctx(N, primes, knobs)
    rng = np.random.default_rng(len(bits))
    _check_key_switches(g, o, primes, rng, "qm1")
    g.close()


# the same words on ntt_modup_kernel: EVAH_FUSE_SMALL=0 sends every key switch past the small-launch form.  l = 1 (one digit,
# whose only job is the special row), both sides of MAC3's first fold (7 | 8) and of its gate (15 | 16), the 128-bit path's
# first fold (15 | 16 | 17); l = 30 and 31 are not repeated, the n = 2 calls of the cases above reach the kernel already
MODUP_CHAINS = [c for c in CHAINS if len(c[2]) - 1 in (1, 7, 8, 15, 16, 17)]


@pytest.mark.parametrize("name,N,bits,knobs", MODUP_CHAINS, ids=[c[0] for c in MODUP_CHAINS])
def test_key_switch_forms_on_the_mod_up_kernel(name, N, bits, knobs):
    primes = po.coeff_modulus_create(N, bits)
    o = po.Oracle(N, primes)
    g = _ctx(N, primes, dict(knobs, EVAH_FUSE_SMALL=0))
    rng = np.random.default_rng(len(bits))
    _check_key_switches(g, o, primes, rng, "qm1", launches=MODUP_LAUNCHES)
    g.close()


def _special_chains(N=4096):
    c60 = po.coeff_modulus_create(N, [60] * 5)
    below54 = _ntt_prime_below((1 << 54) - (1 << 36), N)  # not of the top-bit shape: MAC3 with an unreduced row
    nontb55 = _ntt_prime_below((1 << 55) - (1 << 40), N)  # not of the top-bit shape, above 2^54: the 128-bit path
    return [
        ("below54", N, [c60[0], below54, c60[1], _ntt_prime_below(below54, N), c60[4]]),
        ("nontb55", N, [c60[0], nontb55, c60[1], c60[4]]),
        ("bits30_40", N, po.coeff_modulus_create(N, [40, 30, 40, 30, 40])),
    ]


SPECIAL = _special_chains()


@pytest.mark.parametrize("name,N,primes", SPECIAL, ids=[s[0] for s in SPECIAL])
@pytest.mark.parametrize("key_kind", ["qm1", "mixed"])
def test_key_switch_forms_on_other_prime_shapes(name, N, primes, key_kind):
    o = po.Oracle(N, primes)
    for knobs in ({}, {"EVAH_MAC3": 0}):
        g = _ctx(N, primes, knobs)
        _check_key_switches(g, o, primes, np.random.default_rng(5), key_kind)
        g.close()


@pytest.mark.parametrize("name,N,primes", SPECIAL, ids=[s[0] for s in SPECIAL])
@pytest.mark.parametrize("key_kind", ["qm1", "mixed"])
def test_other_prime_shapes_on_the_mod_up_kernel(name, N, primes, key_kind):
    """compare-and-subtract butterflies and MAC3's unreduced rows behind the mod-up kernel's conversion"""
    o = po.Oracle(N, primes)
    for knobs in ({}, {"EVAH_MAC3": 0}):
        g = _ctx(N, primes, dict(knobs, EVAH_FUSE_SMALL=0))
        _check_key_switches(g, o, primes, np.random.default_rng(5), key_kind, launches=MODUP_LAUNCHES)
        g.close()


def boundary_chains(N=4096):
    """Chains around the digit conversion's rule (OpKsDigit::setup): digit t_J < q_J enters the forward rounds under q_kappa
    unreduced when q_J <= 8 q_kappa, through a Barrett reduction otherwise.  p is a 57-bit prime, qA the largest NTT prime
    <= 8 p (lazy under p, by the narrowest margin: with the dense_max and qm1 words its digits are qA - 1, about 8 p, the
    largest value the rule ever lets into the rounds), qB the smallest one > 8 p (reduced under p, by the narrowest
    margin).  None of p, qA, qB has the top-bit shape and all are above 2^54, so these chains take the compare-and-subtract
    butterflies and the 128-bit inner products whatever EVAH_MAC3 says.  Rows (output prime: lazy digits | reduced digits):
      [qA, p, qB, special]       qA: p qB |  -      p: qA | qB      qB: qA p | -      special: qA p qB | -
      [p, qA, p2, qB, special]   p: qA p2 | qB      qA: p p2 qB | -      p2: p | qA qB      qB: p qA p2 | -
                                 special: all | -
    so the workgroup of digit qA (and of digit qB) switches between the two conversions from row to row.
    -> {name: primes}, and (p, p2, qA, qB, special)"""
    p = _ntt_prime_below(3 << 55, N)
    qA = _ntt_prime_below(8 * p + 1, N)
    qB = _ntt_prime_above(8 * p, N)
    # the largest NTT prime with 8 p2 < qA (row "p2: p | qA qB"); at N = 2048 the prime next below p is 4096 away and misses it
    p2 = _ntt_prime_below((qA - 1) // 8 + 1, N)
    special = next(q for q in po.coeff_modulus_create(N, [60] * 3) if q not in (p, p2, qA, qB))
    return {"qA_p_qB": [qA, p, qB, special], "p_qA_p2_qB": [p, qA, p2, qB, special]}, (p, p2, qA, qB, special)


BOUNDARY = boundary_chains()[0]


@pytest.mark.parametrize("chain", sorted(BOUNDARY))
@pytest.mark.parametrize("form", ["small", "modup"])
def test_digit_conversion_at_the_lazy_flag_boundary(chain, form):
    """every key-switch form on the BOUNDARY chains, keys at q - 1, in the small-launch form (ntt_inv_fwd_kernel) and on the
    mod-up kernel, EVAH_MAC3 at its default and 0 (the same kernels here, see boundary_chains: kept because the issue of
    this test asks for both)"""
    N, primes = 4096, BOUNDARY[chain]
    o = po.Oracle(N, primes)
    for knobs in ({}, {"EVAH_MAC3": 0}):
        if form == "modup":
            knobs = dict(knobs, EVAH_FUSE_SMALL=0)
        g = _ctx(N, primes, knobs)
        _check_key_switches(g, o, primes, np.random.default_rng(7), "qm1", launches=MODUP_LAUNCHES if form == "modup" else None)
        g.close()


@pytest.mark.parametrize("N,l", [(65536, 15), (131072, 3)])
def test_key_switch_at_large_degree(N, l):
    """N = 65536 at l = 15: the largest MAC3 shape at the benchmark's degree; one N = 131072 case"""
    primes = po.coeff_modulus_create(N, [60] * (l + 1))
    o = po.Oracle(N, primes)
    g = _ctx(N, primes, {})
    rk = _keys(primes, l, N, None, "qm1")
    g.upload_relin_key(rk)
    div = 60
    for name, p in _forms(o, primes, l, N)[:2]:
        a3 = np.stack([p, p, p])
        A3 = g.upload_ct(a3, 2.0 ** 20)
        want = o.relinearize(a3, rk)
        assert np.array_equal(g.relinearize(A3).download(), want), name
        assert np.array_equal(g.relinearize_rescale(A3, div).download(), o.rescale(want)), name
        a2 = np.stack([p, p])
        A2 = g.upload_ct(a2, 2.0 ** 20)
        assert np.array_equal(g.multiply_rescale_relinearize(A2, A2, div).download(),
                              o.relinearize(o.rescale(o.multiply(a2, a2)), rk)), name
    g.close()


@pytest.mark.parametrize("bits", [[60] * 4, [60, 40, 30, 60], [50, 20, 60]])
def test_rounding_ties_in_rescale_and_mod_down(bits):
    """The dropped limb at 0, (q_last - 1) / 2, (q_last + 1) / 2, q_last - 1: rescale, the fused forms and the chain step"""
    _check_rounding_ties(4096, bits)


def _check_rounding_ties(N, bits):
    primes = po.coeff_modulus_create(N, bits)
    o = po.Oracle(N, primes)
    g = _ctx(N, primes, {})
    k, l = len(primes), len(primes) - 1
    t = _ties(o, primes, l, N)
    rng = np.random.default_rng(9)
    rk = _keys(primes, l, N, rng, "mixed")
    g.upload_relin_key(rk)
    div = int(primes[l - 1]).bit_length()
    a2, a3 = np.stack([t, t]), np.stack([t, t, t])
    A2, A3 = g.upload_ct(a2, 2.0 ** 20), g.upload_ct(a3, 2.0 ** 20)
    assert np.array_equal(g.rescale(A2, div).download(), o.rescale(a2))
    for got in g.rescale_many([A3, A3], div):
        assert np.array_equal(got.download(), o.rescale(a3))
    assert np.array_equal(g.relinearize_rescale(A3, div).download(), o.rescale(o.relinearize(a3, rk)))
    assert np.array_equal(g.rescale_relinearize(A3, div).download(), o.relinearize(o.rescale(a3), rk))
    m = o.multiply(a2, a2)
    assert np.array_equal(g.multiply_relinearize_rescale(A2, A2, div).download(), o.rescale(o.relinearize(m, rk)))
    assert np.array_equal(g.multiply_rescale_relinearize(A2, A2, div).download(), o.relinearize(o.rescale(m), rk))
    # the mod-down's own rounding: a relinearization whose target makes the special-prime row's inner products sit on
    # whatever they sit on for tie digits
    assert np.array_equal(g.relinearize(A3).download(), o.relinearize(a3, rk))
    g.close()


def test_weighted_sum_multiply_and_elementwise_program_at_q_minus_1():
    """weighted_sum with 64 terms of (q - 1) x (q - 1) (the 128-bit sum reduced once), multiply into size 3, and an
    elementwise program whose ciphertext registers are q - 1"""
    N = 4096
    primes = po.coeff_modulus_create(N, [60, 60, 60, 60])
    o = po.Oracle(N, primes)
    g = _ctx(N, primes, {})
    l = len(primes) - 1
    qm1 = np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])
    a2 = np.stack([qm1, qm1])
    A2 = g.upload_ct(a2, 2.0 ** 20)
    P = g.upload_pt(qm1, 2.0 ** 10)
    want = None
    for _ in range(64):
        t = o.multiply_plain(a2, qm1)
        want = t if want is None else o.add(want, t)
    assert np.array_equal(g.weighted_sum([A2] * 64, [P] * 64).download(), want)
    assert np.array_equal(g.multiply(A2, A2).download(), o.multiply(a2, a2))
    # program: v2 = a * a (size 3), v3 = v2 + v2, v4 = -v3, v5 = a - (-a)
    outs = g.elementwise_program([A2, A2], [(13, 0, 1), (11, 2, 2), (10, 3, 0), (10, 0, 0), (12, 0, 5)], [2, 3, 4, 6])
    m = o.multiply(a2, a2)
    s = o.add(m, m)
    for got, w in zip(outs, [m, s, o.negate(s), o.sub(a2, o.negate(a2))]):
        assert np.array_equal(got.download(), w)
    g.close()


def _ntt_prime_sets(N):
    out = []
    for b in (20, 30, 31, 32, 33, 34, 40, 50, 53, 54, 55, 59, 60):
        try:
            out.append(po.coeff_modulus_create(N, [b])[0])
        except Exception:
            pass
    out.append(_ntt_prime_below((1 << 54) - (1 << 36), N))
    out.append(_ntt_prime_below((1 << 55) - (1 << 40), N))
    q16 = (1 << 36) * 16 // 17
    out += [_ntt_prime_below(q16 + (1 << 28), N), _ntt_prime_below(q16 - (1 << 28), N),
            _ntt_prime_below(int(1.2 * 2 ** 32), N), _ntt_prime_below(int(3.05 * 2 ** 32), N)]
    return sorted(set(out))


@pytest.mark.parametrize("logN", range(10, 18))
def test_transforms_on_extreme_inputs(logN):
    """test_ntt forward and inverse at every N from 2^10 to 2^17 on every prime shape: all q - 1, delta at a few
    indices, alternating 0 / q - 1"""
    N = 1 << logN
    primes = _ntt_prime_sets(N)
    o = po.Oracle(N, primes)
    g = backend.Context(N, primes)
    for i, q in enumerate(primes):
        ins = [np.full(N, q - 1, dtype=np.uint64), np.tile(np.array([0, q - 1], dtype=np.uint64), N // 2)]
        for j in (0, 1, N // 2, N - 1):
            d = np.zeros(N, dtype=np.uint64)
            d[j] = q - 1
            ins.append(d)
        for x in ins:
            assert np.array_equal(g.test_ntt(i, x), o.ntt(i, x)), f"ntt N={N} q={q:#x}"
            assert np.array_equal(g.test_ntt(i, x, inverse=True), o.intt(i, x)), f"intt N={N} q={q:#x}"
    g.close()
