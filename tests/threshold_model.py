"""Threshold decryption in Python integers: the flooding noise from the numpy ChaCha20 of the seeded and
sampled tests, a party's share h = c1 s_p + NTT(E), the combination m = c0 + sum_p h_p, and the plain decryption under
s = sum_p s_p that the combination is a flooded form of.  What the CPU and GPU tests compare the host twin and the device
with, word for word.  No test of its own."""
import numpy as np

from pyref import centered, crt
from refresh_model import Chain, intt, ntt
from test_seeded_cpu import chacha20

FLOOD_TAG = 0x666c000000000000
SEED_TAG, SAMPLE_TAG = 0x6331000000000000, 0x736d000000000000   # the tags the flood's must differ from


def flood(fk, sigma, N):
    """E[j] = (w >> (63 - sigma)) - 2^sigma, w = u64 word j % 8 of block j / 8 under FLOOD_TAG: Python integers"""
    blocks = np.arange((N + 7) // 8, dtype=np.uint64)
    w = chacha20(fk, (blocks & 0xFFFFFFFF).astype(np.uint32), (blocks >> 32).astype(np.uint32),
                 FLOOD_TAG & 0xFFFFFFFF, FLOOD_TAG >> 32).astype(np.uint64)
    w64 = (w[:, 0::2] | (w[:, 1::2] << np.uint64(32))).reshape(-1)[:N]
    return [(int(x) >> (63 - sigma)) - (1 << sigma) for x in w64]


def _obj(row):
    return np.array([int(v) for v in row], dtype=object)


def share(ch, ct, sigma, fk, E=None):
    """h [l][N] of the size-2 ciphertext ct [2][l][N] under the key share ch.s: c1 s + NTT(E mod q_i)"""
    _, l, N = ct.shape
    E = flood(fk, sigma, N) if E is None else E
    out = np.empty((l, N), dtype=np.uint64)
    for i in range(l):
        q = ch.primes[i]
        en = ntt([v % q for v in E], ch.psi[i], q)
        out[i] = np.array((_obj(ct[1][i]) * ch.s[i] + en) % q, dtype=np.uint64)
    return out


def combine(ch, ct, shares):
    """m [l][N] = c0 + sum_p h_p in NTT form (ch supplies the primes only)"""
    _, l, N = ct.shape
    out = np.empty((l, N), dtype=np.uint64)
    for i in range(l):
        q = ch.primes[i]
        acc = _obj(ct[0][i])
        for h in shares:
            acc = (acc + _obj(h[i])) % q
        out[i] = np.array(acc, dtype=np.uint64)
    return out


def coefficients(ch, m):
    """m (NTT form) -> coefficient form [l][N], the words the decoder's Garner step reads"""
    l, N = m.shape
    out = np.empty((l, N), dtype=np.uint64)
    for i in range(l):
        out[i] = np.array(intt(m[i], ch.psi[i], ch.primes[i]), dtype=np.uint64)
    return out


def centred_integers(ch, coeff):
    l, N = coeff.shape
    out = []
    for n in range(N):
        U, Q = crt([int(coeff[i][n]) for i in range(l)], ch.primes[:l])
        out.append(centered(U, Q))
    return out


def plain_message(ch_sum, ct):
    """c0 + c1 s under the whole key (ch_sum.s = sum_p s_p), NTT form [l][N]"""
    _, l, N = ct.shape
    out = np.empty((l, N), dtype=np.uint64)
    for i in range(l):
        q = ch_sum.primes[i]
        out[i] = np.array((_obj(ct[0][i]) + _obj(ct[1][i]) * ch_sum.s[i]) % q, dtype=np.uint64)
    return out


def sum_chain(chains):
    """the chain of the collective key: s = sum_p s_p per limb"""
    N, primes = chains[0].N, chains[0].primes
    s = [np.array(sum(c.s[i] for c in chains) % primes[i], dtype=np.uint64) for i in range(len(primes))]
    return Chain(N, primes, s)


def Q_of(primes, l):
    Q = 1
    for q in primes[:l]:
        Q *= int(q)
    return Q


def slot_bound(N, parties, sigma, scale):
    """a slot is a sum of N coefficients times unit-modulus roots over scale: |difference| <= N P 2^sigma / scale"""
    return N * parties * 2.0 ** sigma / scale
