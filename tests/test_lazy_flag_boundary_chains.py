"""The prime chains of test_gpu_extremes.py::test_digit_conversion_at_the_lazy_flag_boundary and of
test_gpu_extremes_degrees.py are what those tests say they are at every degree from 2^10 to 2^17 — checked without a GPU,
so that a change of the prime search cannot quietly move them off the boundary or off their prime shape."""
import pytest

from oracle import pyoracle as po
from test_gpu_extremes import _ntt_prime_below, _special_chains, boundary_chains
from test_gpu_extremes_degrees import CHAIN_PLAN, chains

DEGREES = [1 << logN for logN in range(10, 18)]


def _top_bit_shape(q):
    """the library's rule, restated (evah_ctx_create): q = 2^b - c with b > 32, c < 2^32 and c < q / 16 takes the top-bit
    butterflies; every other prime the compare-and-subtract ones"""
    b = q.bit_length()
    c = (1 << b) - q
    return b > 32 and c < 1 << 32 and c < q >> 4


def test_boundary_chains_straddle_the_lazy_flag():
    _check_boundary_chains(4096)


@pytest.mark.parametrize("N", DEGREES)
def test_boundary_chains_straddle_the_lazy_flag_at_every_degree(N):
    _check_boundary_chains(N)


def _check_boundary_chains(N):
    chains, (p, p2, qA, qB, special) = boundary_chains(N)
    assert qA <= 8 * p < qB
    assert p.bit_length() == 57 and p2 < p
    assert 8 * p2 < qA  # the digit of qA is reduced under p2 (the rows listed in boundary_chains)
    assert 8 * _ntt_prime_above_strictly(p2, N) >= qA  # ... by the narrowest margin: p2 is the largest such prime
    # every other row of boundary_chains' table: lazy (q_J <= 8 q_kappa) unless listed as reduced
    reduced = {(qB, p), (qA, p2), (qB, p2)}  # (digit prime, output prime)
    for primes in chains.values():
        for qJ in primes[:-1]:
            for qk in primes:
                assert (qJ > 8 * qk) == ((qJ, qk) in reduced), (qJ, qk)
    # no NTT prime lies between qA and qB: the margins are the narrowest there are
    assert all(not po.lib.evo_is_prime(q) for q in range(qA + 2 * N, qB, 2 * N))
    assert len({p, p2, qA, qB, special}) == 5
    for q in (p, p2, qA, qB, special):
        assert q % (2 * N) == 1 and q < 1 << 60 and po.lib.evo_is_prime(q)
    # compare-and-subtract butterflies and the 128-bit inner products on every data prime; the special prime as usual
    for q in (p, p2, qA, qB):
        assert not _top_bit_shape(q) and q > 1 << 54
    assert _top_bit_shape(special)
    assert chains == {"qA_p_qB": [qA, p, qB, special], "p_qA_p2_qB": [p, qA, p2, qB, special]}
    for primes in chains.values():
        o = po.Oracle(N, primes)
        assert o.N == N


def _ntt_prime_above_strictly(q, N):
    q += 2 * N
    while not po.lib.evo_is_prime(q):
        q += 2 * N
    return q


def test_the_chain_at_4096_is_the_one_it_was():
    """p2 used to be the NTT prime next below p; the rule "largest with 8 p2 < qA" picks the same prime at N = 4096"""
    _, (p, p2, _, _, _) = boundary_chains(4096)
    assert p2 == _ntt_prime_below(p, 4096)


@pytest.mark.parametrize("N", DEGREES)
def test_special_chains_keep_their_prime_shapes(N):
    chains = {name: primes for name, n, primes in _special_chains(N) if n == N}
    assert sorted(chains) == ["below54", "bits30_40", "nontb55"]
    for primes in chains.values():
        assert len(set(primes)) == len(primes)
        assert all(q % (2 * N) == 1 and q < 1 << 60 and po.lib.evo_is_prime(q) for q in primes)
        assert _top_bit_shape(primes[-1])
    # MAC3 with unreduced rows: two primes below 2^54 of no top-bit shape, the others with it, and the unreduced digit
    # (below (16 + 4 * 8) q after the 8 contiguous stages of N = 2^16 and 2^17) under the 2^60 of the radix-2^30 split
    b = chains["below54"]
    below54, lower = b[1], b[3]
    assert lower < below54 < 1 << 54 and lower == _ntt_prime_below(below54, N)
    assert not _top_bit_shape(below54) and not _top_bit_shape(lower)
    assert 48 * below54 < 1 << 60
    assert all(_top_bit_shape(q) for q in (b[0], b[2], b[4]))
    # the 128-bit path: one prime above 2^54 of no top-bit shape
    n = chains["nontb55"]
    assert n[1] > 1 << 54 and not _top_bit_shape(n[1])
    assert all(_top_bit_shape(q) for q in (n[0], n[2], n[3]))
    # a 40-bit digit under a 30-bit prime: the digit conversion's Barrett reduction.  The 40-bit primes have the top-bit
    # shape, the 30-bit ones cannot (it starts at 33 bits)
    s = chains["bits30_40"]
    assert [q.bit_length() for q in s] == [40, 30, 40, 30, 40]
    assert [_top_bit_shape(q) for q in s] == [True, False, True, False, True]
    assert max(s[:-1]) > 8 * min(s)


@pytest.mark.parametrize("N", DEGREES)
def test_mod_up_variants_expected_of_the_chains(N):
    """the (top-bit only, lazy only) flags test_gpu_extremes_degrees.py expects of Context.modup_variant(), from the
    library's rules restated: every prime of the top-bit shape / and q_J <= 8 q_kappa for every digit and output prime"""
    for name, primes in chains(N).items():
        tb = all(_top_bit_shape(q) for q in primes)
        lazy = all(qJ <= 8 * qk for qJ in primes[:-1] for qk in primes)
        assert CHAIN_PLAN[name][3] == (tb, tb and lazy), name
    c = chains(N)
    assert all(_top_bit_shape(q) for q in c["c60"]) and len(set(c["c60"])) == 4
    assert [q.bit_length() for q in c["bits34_40"]] == [40, 34, 40, 34, 40]
