"""The stored inputs of lazy_bound_words.py do what test_gpu_extremes_degrees.py feeds them to the GPU for — checked in exact
arithmetic against today's primes and twiddles, without a GPU."""
import numpy as np
import pytest

import lazy_bound_words as lb
from oracle import pyoracle as po


def _first_pass(N):
    primes = po.coeff_modulus_create(N, [60] * 4)
    return primes, po.Oracle(N, primes).root_powers(lb.OUTPUT), (N.bit_length() - 1 + 1) // 2


def test_the_restated_butterflies_compute_the_oracles_transform():
    """all log2 N stages of the restatement, reducing on every stage or on every third, against the oracle's NTT"""
    N = 1024
    primes, rp, _ = _first_pass(N)
    q = primes[lb.OUTPUT]
    x = np.random.default_rng(3).integers(0, q, size=(2, N), dtype=np.uint64)
    for schedule in (lambda s: True, lambda s: s % 3 == 1):
        y = lb.forward_stages(x, q, rp, 10, schedule)
        for a, b in zip(x, y):
            assert [int(v) % q for v in b] == [int(v) for v in po.Oracle(N, primes).ntt(lb.OUTPUT, a)]


@pytest.mark.parametrize("logN", lb.LOG_DEGREES)
def test_stored_inputs_reach_the_bound_and_expose_a_late_reduction(logN):
    N = 1 << logN
    primes, rp, P = _first_pass(N)
    q, r = primes[lb.OUTPUT], lb.run_start(P)
    vecs = lb.stored_vectors(N)
    assert vecs.shape[1] == 1 << P and len(vecs) >= 1 and vecs.max() < primes[lb.DIGIT]
    true = lambda s: lb.tb_reduce_stage_first_pass(P, s)
    late = lambda s: true(s) if s not in (r + 3, r + 4) else s == r + 4  # the reduction of stage r + 3 one stage late
    assert r + 4 < P
    for v in vecs:
        # the true schedule stays below 16 q (asserted inside), and stage r + 3 would leave a value of 2^64 or more
        assert lb.late_value_exact(v, q, rp, P) >= 1 << 64
        good = [int(x) % q for x in lb.forward_stages(v[None, :], q, rp, P, true)[0]]
        bad = [int(x) % q for x in lb.forward_stages(v[None, :], q, rp, P, late)[0]]
        assert good != bad  # the wrapped word is another residue: a result computed that way differs from the oracle's
