"""The collective relinearization-key generation in Python integers: the seed derivation from the numpy
ChaCha20 of the seeded tests, the common rows and the small polynomials from their numpy restatements, both rounds, the
aggregate, the key, the key equation over the integers and the bounds that follow from it.  What the CPU and GPU tests
compare the host twins and the device with, word for word.  No test of its own.

The contract, with w_J[i] = [i == J] (P mod q_J), a_J[i] = the expansion of seed'_J under prime i, all rows NTT form:
    seed'_J  = the first 32 bytes of the ChaCha20 block keyed by relin.seeds[J], counter 0, nonce "evarlk\\0\\0"
    round 1  h0[J][i] = -(a_J[i] u_J[i]) + NTT_i(e0_J) + w_J[i] s[i]        h1[J][i] = a_J[i] s[i] + NTT_i(e1_J)
    round 2  g[J][i]  = s[i] H0[J][i] + NTT_i(e2_J) + (u_J[i] - s[i]) H1[J][i] + NTT_i(e3_J)
    key      (c0, c1) = (sum_p g_p[J], H1[J]):  c0 + c1 s = w_J s^2 + s e0 + u e1 + e2 + e3 over the sums of the parties
with (u_J, e0_J, e1_J) = small(r1[J], 0 / 1 / 2) and (e2_J, e3_J) = small(r2[J], 1 / 2)."""
import struct

import numpy as np

from pyref import centered, crt
from refresh_model import intt, ntt
from test_sampled_cpu import expand_small
from test_seeded_cpu import chacha20, expand_limb

ROUND_NONCE = b"evarlk\0\0"
COMMON_NONCE = b"evacrs\0\0"   # the nonce of the common public stream, which this one must differ from
ERR_MAX = 21   # a sampled error is a difference of two 21-bit popcounts: the B of DESIGN.md 1.15


def derive_seed(relin_seed):
    w14, w15 = struct.unpack("<II", ROUND_NONCE)
    return chacha20(bytes(relin_seed), 0, 0, w14, w15)[0].astype("<u4").tobytes()[:32]


def derive_seeds(relin_seeds):
    """[D][32] uint8 -> [D][32] uint8"""
    return np.stack([np.frombuffer(derive_seed(bytes(s)), dtype=np.uint8) for s in np.asarray(relin_seeds, dtype=np.uint8)])


def _obj(row):
    return np.array([int(v) for v in row], dtype=object)


def _small_ntt(ch, i, small):
    q = ch.primes[i]
    return ntt([int(v) % q for v in small], ch.psi[i], q)


def round1(ch, seeds, r1keys):
    """[D][2][k][N] of the party whose key share is ch.s"""
    N, k, D = ch.N, len(ch.primes), len(r1keys)
    P = ch.primes[-1]
    out = np.empty((D, 2, k, N), dtype=np.uint64)
    for J in range(D):
        u, e0, e1 = (expand_small(bytes(r1keys[J]), p, N) for p in range(3))
        for i, q in enumerate(ch.primes):
            a = _obj(expand_limb(bytes(seeds[J]), i, q, N))
            h0 = (-(a * _small_ntt(ch, i, u)) + _small_ntt(ch, i, e0)) % q
            if i == J:
                h0 = (h0 + (P % q) * ch.s[i]) % q
            out[J, 0, i] = np.array(h0, dtype=np.uint64)
            out[J, 1, i] = np.array((a * ch.s[i] + _small_ntt(ch, i, e1)) % q, dtype=np.uint64)
    return out


def aggregate(shares, primes):
    """row-by-row sums of arrays [...][k][N]"""
    k = len(primes)
    acc = np.zeros(shares[0].shape, dtype=object)
    for s in shares:
        acc = acc + s.astype(object)
    flat = acc.reshape(-1, k, acc.shape[-1])
    for i, q in enumerate(primes):
        flat[:, i, :] %= int(q)
    return np.array(flat.reshape(shares[0].shape), dtype=np.uint64)


def round2(ch, agg, r1keys, r2keys):
    """[D][k][N]"""
    N, k, D = ch.N, len(ch.primes), len(r1keys)
    out = np.empty((D, k, N), dtype=np.uint64)
    for J in range(D):
        u = expand_small(bytes(r1keys[J]), 0, N)
        e2, e3 = expand_small(bytes(r2keys[J]), 1, N), expand_small(bytes(r2keys[J]), 2, N)
        for i, q in enumerate(ch.primes):
            g = ch.s[i] * _obj(agg[J, 0, i]) + _small_ntt(ch, i, e2) + (_small_ntt(ch, i, u) - ch.s[i]) * _obj(agg[J, 1, i]) + _small_ntt(ch, i, e3)
            out[J, i] = np.array(g % q, dtype=np.uint64)
    return out


def key(agg, round2_shares, primes):
    """[D][2][k][N]: (sum_p g_p, H1)"""
    out = np.empty(agg.shape, dtype=np.uint64)
    out[:, 0] = aggregate(round2_shares, primes)
    out[:, 1] = agg[:, 1]
    return out


def key_noise_integers(ch_sum, key_words, J):
    """the centred integers of c0 + c1 s - w_J s^2 of digit J over the key level (all k primes), s = ch_sum.s"""
    k, N = len(ch_sum.primes), ch_sum.N
    P = ch_sum.primes[-1]
    rows = []
    for i, q in enumerate(ch_sum.primes):
        s = ch_sum.s[i]
        m = _obj(key_words[J, 0, i]) + _obj(key_words[J, 1, i]) * s
        if i == J:
            m = m - (P % q) * s * s
        rows.append(intt(m % q, ch_sum.psi[i], q))
    out = []
    for n in range(N):
        U, Q = crt([int(rows[i][n]) for i in range(k)], ch_sum.primes)
        out.append(centered(U, Q))
    return out


def key_noise_bound(N, parties, B=ERR_MAX):
    """|s e0 + u e1 + e2 + e3| per coefficient: s, u sums of P ternaries, e. sums of P errors within B, products over N terms"""
    return 2 * N * B * parties * parties + 2 * B * parties


def relin_noise_bound(N, primes, l, parties, B=ERR_MAX):
    """what a relinearization at l limbs with the collective key may add to a coefficient of the decryption under s:
    sum over l digits of d2_J E_J — N terms, |d2_J| < q_J, |E_J| within the key's bound — divided by the special prime, plus
    the mod-down's rounding (1 + N |s|_inf) / 2 per polynomial, |s|_inf <= P, taken whole: N P + 1"""
    qmax = max(int(q) for q in primes[:l])
    return l * N * qmax * key_noise_bound(N, parties, B) // int(primes[-1]) + 1 + N * parties + 1
