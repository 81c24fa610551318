"""The refresh in Python integers: decrypt, recompose with the CRT, centre, divide by 2^t with ties towards
+infinity, reduce under the target primes and encrypt again.  What the CPU and GPU tests of the refresh compare the host twin
and the device with, word for word.  No test of its own.

The transforms are exact radix-2 recursions over Python integers (numpy object arrays); test_refresh_cpu.py pins them to
pyref.naive_ntt once."""
import numpy as np

from eva_amd import _eva
from pyref import bitrev, centered, crt
from test_seeded_cpu import expand_limb

sampled_small = _eva._seal._sampled_small


def minimal_psi(N, q):
    """the numerically smallest primitive 2N-th root of unity mod q (hostmath.h minimal_primitive_root)"""
    e = (q - 1) // (2 * N)
    g = 2
    while pow(pow(g, e, q), N, q) != q - 1:
        g += 1
    root = pow(g, e, q)
    sq, cur, best = root * root % q, root, root
    for _ in range(N):
        best = min(best, cur)
        cur = cur * sq % q
    return best


def _dft(x, w, q):
    """X[k] = sum_j x_j w^(jk) mod q, natural order in and out"""
    n = len(x)
    if n == 1:
        return x
    w2 = w * w % q
    ev, od = _dft(x[0::2], w2, q), _dft(x[1::2], w2, q)
    tw = np.empty(n // 2, dtype=object)
    p = 1
    for k in range(n // 2):
        tw[k] = p
        p = p * w % q
    t = od * tw % q
    return np.concatenate([(ev + t) % q, (ev - t) % q])


def _powers(b, n, q):
    out = np.empty(n, dtype=object)
    p = 1
    for j in range(n):
        out[j] = p
        p = p * b % q
    return out


def ntt(a, psi, q):
    """pyref.naive_ntt: out[i] = sum_j a_j psi^((2 br(i) + 1) j) mod q"""
    n = len(a)
    logn = n.bit_length() - 1
    x = np.array([int(v) for v in a], dtype=object) * _powers(psi, n, q) % q
    X = _dft(x, psi * psi % q, q)
    return np.array([X[bitrev(i, logn)] for i in range(n)], dtype=object)


def intt(A, psi, q):
    n = len(A)
    logn = n.bit_length() - 1
    X = np.empty(n, dtype=object)
    for i in range(n):
        X[bitrev(i, logn)] = int(A[i])
    ipsi = pow(psi, -1, q)
    x = _dft(X, ipsi * ipsi % q, q)
    return x * _powers(ipsi, n, q) % q * pow(n, -1, q) % q


class Chain:
    """the primes of a context with their roots, and the secret key in NTT form [k][N]"""

    def __init__(self, N, primes, s_ntt):
        self.N, self.primes = N, [int(q) for q in primes]
        self.psi = [minimal_psi(N, q) for q in self.primes]
        self.s = [np.array([int(v) for v in row], dtype=object) for row in s_ntt]


def decrypt_integers(ch, ct):
    """the centred integers M[n] of ct [size][l][N] (NTT form): step 1-3 of the contract"""
    size, l, N = ct.shape
    rows = []
    for i in range(l):
        q, s = ch.primes[i], ch.s[i]
        acc = np.array([int(v) for v in ct[0][i]], dtype=object)
        sp = s
        for p in range(1, size):
            acc = (acc + np.array([int(v) for v in ct[p][i]], dtype=object) * sp) % q
            sp = sp * s % q
        rows.append(intt(acc, ch.psi[i], q))
    out = []
    for n in range(N):
        U, Q = crt([rows[i][n] for i in range(l)], ch.primes[:l])
        out.append(centered(U, Q))
    return out


def divide(M, t):
    """floor((M + 2^(t-1)) / 2^t): ties towards +infinity (Python's >> floors)"""
    return M if t == 0 else (M + (1 << (t - 1))) >> t


def encrypt_integers(ch, Mp, L, ek, seed):
    """the symmetric encryption [2][L][N] of the integer polynomial Mp: e = sampled_small(ek, 1), c1 from seed"""
    N = ch.N
    e = [int(v) for v in sampled_small(bytes(ek), 1, N)]
    out = np.empty((2, L, N), dtype=np.uint64)
    for j in range(L):
        q = ch.primes[j]
        m = ntt([v % q for v in Mp], ch.psi[j], q)
        en = ntt([v % q for v in e], ch.psi[j], q)
        a = expand_limb(bytes(seed), j, q, N)
        ao = np.array([int(v) for v in a], dtype=object)
        out[0][j] = np.array((m - (ao * ch.s[j] + en)) % q, dtype=np.uint64)
        out[1][j] = a
    return out


def refresh(ch, ct, L, t, ek, seed, M=None):
    M = decrypt_integers(ch, ct) if M is None else M
    return encrypt_integers(ch, [divide(v, t) for v in M], L, ek, seed)


def message_ciphertext(ch, M, l):
    """a size-2 ciphertext [2][l][N] with c1 = 0 and c0 = NTT(M mod q_i): it decrypts to exactly M"""
    N = ch.N
    out = np.zeros((2, l, N), dtype=np.uint64)
    for i in range(l):
        q = ch.primes[i]
        out[0][i] = np.array(ntt([v % q for v in M], ch.psi[i], q), dtype=np.uint64)
    return out
