"""The prime chains of test_gpu_extremes.py::test_digit_conversion_at_the_lazy_flag_boundary are what that test says they
are — checked without a GPU, so that a change of the prime search cannot quietly move them off the boundary."""
from oracle import pyoracle as po
from test_gpu_extremes import boundary_chains


def test_boundary_chains_straddle_the_lazy_flag():
    N = 4096
    chains, (p, p2, qA, qB, special) = boundary_chains(N)
    assert qA <= 8 * p < qB
    assert p.bit_length() == 57 and p2 < p
    assert 8 * p2 < qA  # the digit of qA is reduced under p2 (the rows listed in boundary_chains)
    # no NTT prime lies between qA and qB: the margins are the narrowest there are
    assert all(not po.lib.evo_is_prime(q) for q in range(qA + 2 * N, qB, 2 * N))
    assert len({p, p2, qA, qB, special}) == 5
    for q in (p, p2, qA, qB, special):
        assert q % (2 * N) == 1 and q < 1 << 60 and po.lib.evo_is_prime(q)
    assert chains == {"qA_p_qB": [qA, p, qB, special], "p_qA_p2_qB": [p, qA, p2, qB, special]}
    for primes in chains.values():
        o = po.Oracle(N, primes)
        assert o.N == N
