"""The worst-case words of test_gpu_extremes.py at every transform pass shape, not only N = 4096.

Every fused transform kernel is compiled per pass size P: the launch layer splits logN into a strided pass of
P_a = (logN + 1) / 2 stages and a contiguous pass of P_b = logN / 2 stages,
    N      2^10   2^11   2^12   2^13   2^14   2^15   2^16   2^17
    (a,b)  (5,5)  (6,5)  (6,6)  (7,6)  (7,7)  (8,7)  (8,8)  (9,8)
and what depends on P is what the lazy arithmetic rests on: the stages on which the top-bit butterflies reduce
(tb_reduce_stage: s = P - 2 mod 3, with an extra clause for P = 7), the growth of the rows that ks_inner_kernel<MAC3>
never reduces (below (16 + 4 P_b) q: tightest at P_b = 8), the column tiles of ntt_modup_kernel (2^(11 - P) columns wide)
and the LDS padding.  test_gpu_extremes.py covers (6,6); this module runs the same check (_check_key_switches: keys at
q - 1, every key-switch form, single, _many and batched) at the seven other degrees, on these chains (3 data limbs plus
the special prime unless stated):
  c60        [60] * 4: top-bit primes, the fully specialised mod-up kernel; EVAH_MAC3 at its default and 0
  below54    two primes below 2^54 of no top-bit shape: MAC3 with unreduced rows; EVAH_MAC3 at its default and 0
  nontb55    a prime above 2^54 of no top-bit shape: compare-and-subtract butterflies, 128-bit inner products
  bits30_40  [40, 30, 40, 30, 40]: digits above 8 q_kappa (the Barrett conversion); a 30-bit prime has no top-bit shape
             either (the shape needs more than 32 bits), so the mod-up kernel is the generic one and MAC3 runs its rows
             unreduced
  bits34_40  [40, 34, 40, 34, 40], mod-up forms only: the same with every prime of the top-bit shape, which is the one
             chain here whose mod-up kernel is "top-bit only" (both digit conversions compiled in)
  qA_p_qB, p_qA_p2_qB   boundary_chains(N): both sides of the digit conversion's rule q_J <= 8 q_kappa
in these launch forms, each proved by the launch counts of one relinearize (an id whose kernel did not run fails):
  small_lr2, small_lr3   ntt_inv_fwd_kernel / ntt_inv2_kernel, forced with EVAH_FUSE_SMALL far above any tile count, at
             both EVAH_SMALL_LR; small_lr2 also lifts EVAH_CHAIN_FUSE_BLOCKS, so the chain step's digit launch is the
             fused one at every degree (at its default it is from 2^16 down, single calls only)
  modup, modup_lr2, modup_spec0   ntt_modup_kernel (EVAH_FUSE_SMALL=0), in the variant Context.modup_variant() reports,
             which is asserted per chain
  two_launch the plain passes behind the ops' lazy loads (EVAH_FUSE_SMALL=0 EVAH_MODUP=0): c60 and below54 only.
N = 1024 has neither fused form (partial tiles): there the default two-launch form is the case, for every chain.
Word forms: all four up to 2^14; qm1 and dense_max, which put every digit at its own prime's maximum, from 2^15 up.
What these words do NOT do is come near the growth of 4 q per stage that the reduction schedules budget for: a constant
polynomial's lazy zeros give twiddle products of q, 2 q or 3 q, and a scratch build with one reduction stage of P = 7
moved (or tb_reduce_stage's s == 0 clause dropped) passed every case on them.  The c60 chain therefore also runs the
"searched" form (lazy_bound_words.py): digit 0 holds, in every column of the strided pass under prime 1, an input found
by search on which the butterfly of the reducing stage that ends the first full run holds X + 4 q - t >= 2^64, so a
reduction one stage late wraps a word; test_lazy_bound_words.py checks that in exact arithmetic.  That covers the first
(strided) pass of the top-bit butterflies at every P through relinearize and its fused forms.  The contiguous pass's
schedule and the (16 + 4 P_b) q of the unreduced MAC3 rows are NOT pushed to their bounds by any word here: the latter
rests on the check at context creation.
Keys: q - 1, and q - 1 mixed with zeros in addition on below54, nontb55 and bits30_40 (an id each).
The oracle's words do not depend on the knobs: they are computed once per (degree, chain, key kind, word form) and shared
by the launch forms (_Memo), which is why the cases of one chain stand next to each other."""
import functools
import hashlib

import numpy as np
import pytest

from lazy_bound_words import bound_reaching_poly
from oracle import pyoracle as po
from test_gpu_extremes import (MODUP_LAUNCHES, _check_key_switches, _check_rounding_ties, _ctx, _forms, _special_chains,
                               boundary_chains)

pytestmark = pytest.mark.gpu

LOG_DEGREES = [10, 11, 13, 14, 15, 16, 17]


def _counts(**n):
    return {c: n.get(c, 0) for c in MODUP_LAUNCHES}


# one relinearize of a stored size-3 ciphertext (MODUP_LAUNCHES is the mod-up kernel's):
# small-launch form: contiguous inverse pass, ntt_inv_fwd_kernel (ksdigit_pass1), the key-switch kernel with the special
# rows' first inverse pass inside it, ntt_inv_fwd_kernel of the mod-down (moddown_pass1), its second pass
SMALL_LAUNCHES = _counts(intt_pass1=1, ksdigit_pass1=1, ks_mac=1, moddown_pass1=1, moddown_pass2=1)
# two-launch form: both inverse passes of the digits and of the special rows, each forward pass on its own
TWO_LAUNCHES = _counts(intt_pass1=2, intt_pass2=2, ksdigit_pass1=1, ks_mac=1, moddown_pass1=1, moddown_pass2=1)
assert len({tuple(sorted(d.items())) for d in (SMALL_LAUNCHES, TWO_LAUNCHES, MODUP_LAUNCHES)}) == 3

BIG = 1 << 30
# small_lr2 lifts EVAH_CHAIN_FUSE_BLOCKS too: without it the chain step never takes its fused digit launch (OpChainDigit in
# ntt_inv2_kernel) at 2^17; small_lr3 keeps that knob at its default
# name -> (knobs, launch counts of one relinearize, EVAH_MODUP_LR / EVAH_MODUP_SPEC of a mod-up form)
FORMS = {
    "small_lr2": ({"EVAH_FUSE_SMALL": BIG, "EVAH_SMALL_LR": 2, "EVAH_CHAIN_FUSE_BLOCKS": BIG}, SMALL_LAUNCHES, None),
    "small_lr3": ({"EVAH_FUSE_SMALL": BIG, "EVAH_SMALL_LR": 3}, SMALL_LAUNCHES, None),
    "modup": ({"EVAH_FUSE_SMALL": 0}, MODUP_LAUNCHES, (3, 1)),
    "modup_lr2": ({"EVAH_FUSE_SMALL": 0, "EVAH_MODUP_LR": 2}, MODUP_LAUNCHES, (2, 1)),
    "modup_spec0": ({"EVAH_FUSE_SMALL": 0, "EVAH_MODUP_SPEC": 0}, MODUP_LAUNCHES, (3, 0)),
    "two_launch": ({"EVAH_FUSE_SMALL": 0, "EVAH_MODUP": 0}, TWO_LAUNCHES, None),
    "default": ({}, TWO_LAUNCHES, None),  # N = 1024 only
}
FUSED = ["small_lr2", "small_lr3", "modup", "modup_lr2", "modup_spec0"]
MODUP = ["modup", "modup_lr2", "modup_spec0"]

# chain -> (EVAH_MAC3 settings, key kinds, launch forms at N >= 2048,
#           (top-bit only, lazy only) of the specialised mod-up kernel: test_lazy_flag_boundary_chains.py checks these
#           against the library's rules at every degree)
CHAIN_PLAN = {
    "c60": ((None, 0), ("qm1",), FUSED + ["two_launch"], (True, True)),
    "below54": ((None, 0), ("qm1", "mixed"), FUSED + ["two_launch"], (False, False)),
    "nontb55": ((None,), ("qm1", "mixed"), FUSED, (False, False)),
    "bits30_40": ((None,), ("qm1", "mixed"), FUSED, (False, False)),
    "bits34_40": ((None,), ("qm1",), MODUP, (True, False)),
    "qA_p_qB": ((None,), ("qm1",), FUSED, (False, False)),
    "p_qA_p2_qB": ((None,), ("qm1",), FUSED, (False, False)),
}


@functools.lru_cache(maxsize=None)
def chains(N):
    """{chain name: primes} at degree N, in CHAIN_PLAN's order"""
    out = {"c60": po.coeff_modulus_create(N, [60] * 4)}
    out.update({name: primes for name, _, primes in _special_chains(N)})
    out["bits34_40"] = po.coeff_modulus_create(N, [40, 34, 40, 34, 40])
    out.update(boundary_chains(N)[0])
    assert list(out) == list(CHAIN_PLAN)
    return out


def _cases():
    """(id, logN, chain, knobs, form, key kind): a chain's cases next to each other, so that the oracle's words are shared"""
    out = []
    for logN in LOG_DEGREES:
        for chain, (mac3s, key_kinds, forms, _) in CHAIN_PLAN.items():
            if logN == 10:
                forms = ["default"] if chain != "bits34_40" else []
            for mac3 in mac3s:
                for form in forms:
                    for kind in key_kinds:
                        out.append((f"N{1 << logN}-{chain}{'_mac3off' if mac3 == 0 else ''}-{form}-keys_{kind}", logN, chain,
                                    {} if mac3 is None else {"EVAH_MAC3": 0}, form, kind))
    return out


CASES = _cases()


class _Memo:
    """an Oracle whose methods remember their results by the bytes of their arguments; the results are read-only.
    An argument's digest is remembered by the array object for the length of one test (forget_arrays), so that a key of
    tens of MB is hashed once, not once per call: nothing here or in _check_key_switches writes into an array it made"""

    def __init__(self, o):
        self._o, self.N, self._seen, self._digests = o, o.N, {}, {}

    def forget_arrays(self):
        self._digests.clear()

    def _digest(self, a):
        if not isinstance(a, np.ndarray):
            return a
        if id(a) not in self._digests:  # the entry holds the array, so its id stays its own
            d = hashlib.blake2b(np.ascontiguousarray(a).data, digest_size=16).digest()
            self._digests[id(a)] = (a, (a.shape, a.dtype.str, d))
        return self._digests[id(a)][1]

    def __getattr__(self, name):
        fn = getattr(self._o, name)

        def call(*args):
            key = (name,) + tuple(self._digest(a) for a in args)
            if key not in self._seen:
                r = fn(*args)
                if isinstance(r, np.ndarray):
                    r.flags.writeable = False
                self._seen[key] = r
            return self._seen[key]

        return call


_ORACLE = {}  # the memo of the chain being tested: one (N, primes) at a time, so the stored words stay a few hundred MB


@pytest.fixture(scope="module", autouse=True)
def _drop_the_oracle_words_after_the_module():
    yield
    _ORACLE.clear()


def _oracle(N, primes):
    key = (N, tuple(primes))
    if key not in _ORACLE:
        _ORACLE.clear()
        _ORACLE[key] = _Memo(po.Oracle(N, primes))
    _ORACLE[key].forget_arrays()
    return _ORACLE[key]


def _searched_form(o, primes, N):
    """the polynomial whose digit 0 is bound_reaching_poly(N): relinearize and its fused forms transform it under prime 1
    in the strided pass, where every column then holds a value that a reduction one stage late would wrap"""
    coeff = bound_reaching_poly(N)
    return np.stack([o.ntt(i, coeff % np.uint64(primes[i])) for i in range(len(primes) - 1)])


@pytest.mark.parametrize("name,logN,chain,knobs,form,key_kind", CASES, ids=[c[0] for c in CASES])
def test_key_switch_forms_on_worst_case_words_at_every_pass_shape(name, logN, chain, knobs, form, key_kind):
    N = 1 << logN
    primes = chains(N)[chain]
    spec_flags = CHAIN_PLAN[chain][3]
    form_knobs, launches, modup = FORMS[form]
    o = _oracle(N, primes)
    forms = _forms(o, primes, len(primes) - 1, N)
    if logN >= 15:
        forms = [f for f in forms if f[0] in ("qm1", "dense_max")]
    if chain == "c60":
        forms.append(("searched", _searched_form(o, primes, N)))
    g = _ctx(N, primes, dict(knobs, **form_knobs))
    try:
        if modup is not None:
            lr, spec = modup
            assert g.modup_variant() == ((lr,) + spec_flags if spec else (lr, False, False))
        _check_key_switches(g, o, primes, np.random.default_rng(5), key_kind, forms=forms, launches=launches)
    except AssertionError as e:
        raise AssertionError(f"N=2^{logN} chain {chain} {knobs} form {form} keys {key_kind}: {e}") from e
    finally:
        g.close()
        o.forget_arrays()


@pytest.mark.parametrize("bits", [[60] * 4, [60, 40, 30, 60]], ids=["60x4", "60_40_30_60"])
@pytest.mark.parametrize("logN", LOG_DEGREES)
def test_rounding_ties_at_every_pass_shape(logN, bits):
    """test_rounding_ties_in_rescale_and_mod_down's body: the dropped limb at 0, (q_last -+ 1) / 2 and q_last - 1"""
    _check_rounding_ties(1 << logN, bits)
