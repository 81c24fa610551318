"""The strided passes of the mod-up and tail kernels with their uniform round's twiddles in scalar registers (EVAH_TW_SGPR,
ntt.hip.h: UTw) leave the oracle's words at every strided pass size.

The first forward round of a strided pass, and the last round of its inverse, use heap nodes 1 .. 2^RB - 1 for every thread:
ntt_modup_kernel and ntt_tail_kernel read them, their row's prime and (the tail) the conversion's constants with scalar
loads and name them as scalar operands of the butterflies.  The words must not move, so every case compares with the CPU
oracle word for word, and launch counts prove that the two kernels are what ran.  The kernels are compiled per strided
pass size P_a = (logN + 1) / 2, so the degrees are
    N      2^12   2^13   2^15   2^17
    P_a    6      7      8      9          (rounds of 3+3, 3+2+2, 3+3+2, 3+3+3 stages at 8 coefficients per thread)
with the throughput forms forced on at these small launch sizes (EVAH_MODUP=1, EVAH_TAIL_FUSE=1, EVAH_KS_TAIL=1, and
EVAH_FUSE_SMALL=0, which is what keeps the small-launch form away), on three chains:
  c60      four 60-bit primes: the TBONLY + LAZYONLY instantiations of both kernels;
  mixed    60, 38, 60-bit data primes and a 40-bit special prime (test_gpu_ks_tail.py): every prime has the top-bit shape,
           but the digit and tail conversions take the Barrett form on the rows of the small primes (TBONLY only);
  nontb55  a 55-bit prime of no top-bit shape (test_gpu_extremes.py): the generic instantiations, compare-and-subtract
           butterflies; the key switch is the 128-bit kernel there, so the tail's contiguous passes stay launches of their own.
Words: uniform random; every residue at q - 1 (qm1); every coefficient of limb J at q_J - 1 (dense_max); keys at q - 1 for
the latter two.  Calls: relinearize, relinearize_rescale, multiply_relinearize_rescale_many of two products, and one
rotation through switch_key (a single rotation is never hoisted).  All four degrees are eligible for every form."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

KNOBS = {"EVAH_MODUP": 1, "EVAH_TAIL_FUSE": 1, "EVAH_KS_TAIL": 1, "EVAH_FUSE_SMALL": 0}
STEP = 3


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


def _ntt_prime_below(bound, N):
    q = bound - (bound % (2 * N)) + 1
    while q >= bound or not po.lib.evo_is_prime(q):
        q -= 2 * N
    return q


def _nontb55(N):
    c60 = po.coeff_modulus_create(N, [60] * 5)
    nontb = _ntt_prime_below((1 << 55) - (1 << 40), N)  # 2^55 - c with c >= 2^32, above 2^54: no top-bit shape
    return [c60[0], nontb, c60[1], c60[4]]


# chain -> (primes(N), (top-bit only, lazy only) of the mod-up kernel, the same of the tail kernel,
#           the tail's contiguous passes run inside the key-switch kernel)
CHAINS = {
    "c60": (lambda N: po.coeff_modulus_create(N, [60] * 4), (True, True), (True, True), True),
    "mixed": (lambda N: po.coeff_modulus_create(N, [60, 38, 60, 40]), (True, False), (True, False), True),
    "nontb55": (_nontb55, (False, False), (False, False), False),
}
LOG_DEGREES = [12, 13, 15, 17]
KINDS = ("random", "qm1", "dense_max")
CASES = [(f"N2^{logN}-{chain}-{kind}", logN, chain, kind) for logN in LOG_DEGREES for chain in CHAINS for kind in KINDS]


def _counts(g, call):
    g.profile(True)
    g.profile_reset()
    keep = call()  # the result stays alive until the launches have run
    g.sync()
    del keep
    out = {name: n for name, (n, _) in g.profile_get().items()}
    g.profile(False)
    return out


@pytest.mark.parametrize("name,logN,chain,kind", CASES, ids=[c[0] for c in CASES])
def test_scalar_twiddle_passes_leave_the_oracle_words(name, logN, chain, kind):
    N = 1 << logN
    make, modup_flags, tail_flags, ks_tail = CHAINS[chain]
    primes = make(N)
    k, l = len(primes), len(primes) - 1
    div = int(primes[-2]).bit_length()
    o = po.Oracle(N, primes)
    rng = np.random.default_rng(logN * 16 + k)

    def rand(prefix, nl):
        return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))

    if kind == "random":
        rk, gk = rand((l, 2), k), rand((l, 2), k)
        ops = [(rand((2,), l), rand((2,), l)) for _ in range(2)]
        m = o.multiply(*ops[0])
    else:  # keys at q - 1; every residue (qm1) / every coefficient (dense_max) at q - 1
        rk = gk = np.stack([np.full((l, 2, N), primes[i] - 1, dtype=np.uint64) for i in range(k)], axis=2)
        if kind == "qm1":
            p = np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])
        else:
            p = np.stack([o.ntt(i, np.full(N, primes[i] - 1, dtype=np.uint64)) for i in range(l)])
        ops = [(np.stack([p, p]), np.stack([p, p]))] * 2
        m = np.stack([p, p, p])  # the key-switch target is the worst-case polynomial itself
    a = ops[0][0]
    relin = o.relinearize(m, rk)
    triples = [o.op_triple(x, y, rk) for x, y in (ops if kind == "random" else ops[:1])]
    if kind != "random":
        triples = triples * 2
    want = {
        "relinearize": [relin],
        "relinearize_rescale": [o.rescale(relin)],
        "multiply_relinearize_rescale_many": triples,
        "rotate": [o.rotate(a, STEP, gk)],
    }

    def calls(g):
        M = g.upload_ct(m, 2.0 ** 60)
        A = [g.upload_ct(x, 2.0 ** 30) for x, _ in ops]
        B = [g.upload_ct(y, 2.0 ** 30) for _, y in ops]
        return {
            "relinearize": lambda: [g.relinearize(M)],
            "relinearize_rescale": lambda: [g.relinearize_rescale(M, div)],
            "multiply_relinearize_rescale_many": lambda: g.multiply_relinearize_rescale_many(A, B, div),
            "rotate": lambda: [g.rotate(A[0], STEP)],
        }

    g = _ctx(N, primes, KNOBS)
    try:
        g.upload_relin_key(rk)
        g.upload_galois_key(g.galois_elt_from_step(STEP), gk)
        # the instantiations this chain is here for
        assert g.modup_variant() == (3,) + modup_flags, g.modup_variant()
        assert g.tail_variant() == (True,) + tail_flags, g.tail_variant()
        assert g.ks_tail() == (ks_tail, 0), g.ks_tail()
        c = calls(g)
        for what, call in c.items():
            got = [x.download() for x in call()]
            assert len(got) == len(want[what]), what
            for i, (x, y) in enumerate(zip(got, want[what])):
                assert np.array_equal(x, y), f"{what} [{i}]: differs from the oracle"
        # the mod-up kernel is the key switch's one ksdigit_pass1 launch, with the digits' strided inverse pass inside it:
        # the one intt_pass2 launch left in a relinearize is the special rows' (their mod-down runs as plain passes)
        n = _counts(g, c["relinearize"])
        assert n["ksdigit_pass1"] == 1 and n["ksdigit_pass2"] == 0 and n["intt_pass2"] == 1, n
        n_rot = _counts(g, c["rotate"])
        # the tail kernel is the one moddown_pass1 launch, with both strided inverse passes inside it: no intt_pass2 launch
        # is left; the key switch is two launches where it runs the tail's contiguous passes, and moddown_pass2 is gone
        for what in ("relinearize_rescale", "multiply_relinearize_rescale_many"):
            n = _counts(g, c[what])
            assert n["ksdigit_pass1"] == 1 and n["moddown_pass1"] == 1 and n["intt_pass2"] == 0, (what, n)
            assert (n["ks_mac"], n["moddown_pass2"]) == ((2, 0) if ks_tail else (1, 1)), (what, n)
    finally:
        g.close()
    # the rotation: without the mod-up kernel the digits' strided inverse pass is one more intt_pass2 launch, and no
    # other count moves (the rule of test_gpu_modup.py's ran_on_modup)
    g = _ctx(N, primes, dict(KNOBS, EVAH_MODUP=0))
    try:
        g.upload_galois_key(g.galois_elt_from_step(STEP), gk)
        A = g.upload_ct(a, 2.0 ** 30)
        n = _counts(g, lambda: g.rotate(A, STEP))
        assert n["ksdigit_pass1"] == 1 and n["intt_pass2"] >= 1, n
        assert n_rot == dict(n, intt_pass2=n["intt_pass2"] - 1), (n_rot, n)
    finally:
        g.close()
