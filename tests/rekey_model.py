"""What the re-key tests share: test key pairs made in numpy, the re-key key in Python integers, the key
equation and the hard bound on what a re-key may add to a decryption.  No test of its own.

The contract: for digit J and prime row i
    d[J][0][i] = pkB0_i u_J + NTT_i(e0_J) + [i == J] (P mod q_J) sA_i        d[J][1][i] = pkB1_i u_J + NTT_i(e1_J)
with (u_J, e0_J, e1_J) = sampled_small(rk_J, 0 / 1 / 2).  The transforms are the oracle's (O(N log N)); row_by_pyref()
repeats one row with tests/pyref.py's naive transform, which at O(N^2) in Python is affordable for one row only."""
import numpy as np

import pyref
from sampled_keys import sampled_small

CHAINS = {"mixed": [60, 30, 45, 50, 33, 60], "60x4": [60] * 4}
ERR_MAX = 21  # sample_error is a difference of two 21-bit popcounts


def mulmod(a, b, q):
    return ((a.astype(object) * b.astype(object)) % q).astype(np.uint64)


def addmod(a, b, q):
    return ((a.astype(object) + b.astype(object)) % q).astype(np.uint64)


def residues(o, i, small):
    """NTT form under prime i of a polynomial with small signed coefficients"""
    q = o.primes[i]
    return o.ntt(i, np.array([int(v) % q for v in small], dtype=np.uint64))


class KeyPair:
    """s ternary, pk = (-(a s + e), a) with a uniform and e = sampled_small(., 1): what generate_keys makes, from a numpy
    stream"""

    def __init__(self, o, rng):
        N, k = o.N, o.k
        self.s = rng.integers(-1, 2, size=N)
        self.s_ntt = np.stack([residues(o, i, self.s) for i in range(k)])
        self.e = sampled_small(rng.bytes(32), 1, N)
        pk0, pk1 = [], []
        for i, q in enumerate(o.primes):
            a = rng.integers(0, q, size=N, dtype=np.uint64)
            b = addmod(mulmod(a, self.s_ntt[i], q), residues(o, i, self.e), q)
            pk0.append(((q - b.astype(object)) % q).astype(np.uint64))
            pk1.append(a)
        self.pk = np.stack([np.stack(pk0), np.stack(pk1)])


def model_key(o, pk_b, s_a_ntt, rkeys):
    """the re-key key [D][2][k][N] in Python integers"""
    N, k, primes = o.N, o.k, o.primes
    P = primes[-1]
    out = np.empty((len(rkeys), 2, k, N), dtype=np.uint64)
    for J, rk in enumerate(rkeys):
        u, e0, e1 = (sampled_small(bytes(rk), p, N) for p in range(3))
        for i, q in enumerate(primes):
            un = residues(o, i, u)
            d0 = addmod(mulmod(pk_b[0, i], un, q), residues(o, i, e0), q)
            if i == J:
                d0 = addmod(d0, mulmod(s_a_ntt[i], np.full(N, P % q, dtype=np.uint64), q), q)
            out[J, 0, i] = d0
            out[J, 1, i] = addmod(mulmod(pk_b[1, i], un, q), residues(o, i, e1), q)
    return out


def row_by_pyref(o, pk_b, s_a_ntt, rk, J, i):
    """(d[J][0][i], d[J][1][i]) with pyref.naive_ntt for the three transforms"""
    N, q, P = o.N, o.primes[i], o.primes[-1]
    psi = o.psi(i)
    u, e0, e1 = ([int(v) % q for v in sampled_small(bytes(rk), p, N)] for p in range(3))
    un, e0n, e1n = pyref.naive_ntt(u, psi, q), pyref.naive_ntt(e0, psi, q), pyref.naive_ntt(e1, psi, q)
    f = P % q if i == J else 0
    d0 = [(int(p) * x + e + f * int(s)) % q for p, x, e, s in zip(pk_b[0, i], un, e0n, s_a_ntt[i])]
    d1 = [(int(p) * x + e) % q for p, x, e in zip(pk_b[1, i], un, e1n)]
    return np.array(d0, dtype=np.uint64), np.array(d1, dtype=np.uint64)


def key_noise(o, key, s_a_ntt, s_b_ntt):
    """max over digits and rows of the centred coefficients of c0 + c1 sB - [i == J] P sA: the key equation's left side"""
    N, primes = o.N, o.primes
    P, worst = primes[-1], 0
    for J in range(key.shape[0]):
        for i, q in enumerate(primes):
            m = addmod(key[J, 0, i], mulmod(key[J, 1, i], s_b_ntt[i], q), q)
            if i == J:
                m = ((m.astype(object) - (P % q) * s_a_ntt[i].astype(object)) % q).astype(np.uint64)
            c = o.intt(i, m).astype(object)
            worst = max(worst, max(int(min(v, q - v)) for v in c))
    return worst


def noise_bound(N):
    """|e_pk u| <= 21 N, |e0| <= 21, |e1 sB| <= 21 N"""
    return ERR_MAX * (2 * N + 1)


def slot_bound(N, primes, l, scale_bits):
    """every slot of a re-keyed value within this of the input's own decryption: the key-switch sum — l digits of N terms,
    a digit coefficient below q_J, the key's noise — over P, plus the mod-down's rounding (N + 1 with |sB| <= 1), carried to
    the slots by the decoder's sum of N coefficients, over the scale"""
    qmax = max(primes[:l])
    return N * (l * N * noise_bound(N) * qmax / primes[-1] + N + 1) / 2.0 ** scale_bits
