"""The refresh in Python integers: decrypt, recompose with the CRT, centre, divide by 2^t with ties towards
+infinity, reduce under the target primes and encrypt again.  What the CPU and GPU tests of the refresh compare the host twin
and the device with, word for word.  No test of its own.

The transforms are exact radix-2 passes over Python integers (numpy object arrays) with the powers of each root kept
between calls; test_refresh_cpu.py pins them to pyref.naive_ntt and the recomposition to pyref.crt once."""
import numpy as np

from eva_amd import _eva
from pyref import bitrev, centered
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
    """X[k] = sum_j x_j w^(jk) mod q, natural order in and out: decimation in time, one whole-array step per stage"""
    n = len(x)
    x = x[_bitrev_index(n)]
    m = 1
    while m < n:   # n / 2m transforms of length 2m from their halves: X[k], X[k + m] = E[k] +- w_2m^k O[k]
        x = x.reshape(n // (2 * m), 2, m)
        t = x[:, 1, :] * _powers(pow(w, n // (2 * m), q), m, q) % q
        x = np.concatenate([(x[:, 0, :] + t) % q, (x[:, 0, :] - t) % q], axis=1).reshape(n)
        m *= 2
    return x


_power_tables = {}


def _powers(b, n, q):
    """b^0 .. b^(n-1) mod q in Python integers; kept per (b, n, q): a long chain transforms under one root many times"""
    if (b, n, q) not in _power_tables:
        out = np.empty(n, dtype=object)
        p = 1
        for j in range(n):
            out[j] = p
            p = p * b % q
        _power_tables[(b, n, q)] = out
    return _power_tables[(b, n, q)]


_bitrevs = {}


def _bitrev_index(n):
    if n not in _bitrevs:
        _bitrevs[n] = np.array([bitrev(i, n.bit_length() - 1) for i in range(n)])
    return _bitrevs[n]


def _objects(a):
    out = np.empty(len(a), dtype=object)
    out[:] = [int(v) for v in a]
    return out


def ntt(a, psi, q):
    """pyref.naive_ntt: out[i] = sum_j a_j psi^((2 br(i) + 1) j) mod q"""
    n = len(a)
    x = _objects(a) * _powers(psi, n, q) % q
    X = _dft(x, psi * psi % q, q)
    return X[_bitrev_index(n)]


def intt(A, psi, q):
    n = len(A)
    X = np.empty(n, dtype=object)
    X[_bitrev_index(n)] = _objects(A)
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
    return crt_centered(rows, ch.primes[:l])


def crt_centered(rows, primes):
    """centered(pyref.crt(...)) of every column of rows [l][N], with crt's per-prime constants (Q / q_i) ((Q / q_i)^-1 mod
    q_i) formed once, not once per coefficient (test_refresh_cpu.py pins it to pyref.crt)"""
    Q = 1
    for q in primes:
        Q *= q
    U = np.zeros(len(rows[0]), dtype=object)
    for row, q in zip(rows, primes):
        Qi = Q // q
        U = U + row * (Qi * pow(Qi, -1, q))
    return [centered(int(u), Q) for u in U]


def divide(M, t):
    """floor((M + 2^(t-1)) / 2^t): ties towards +infinity (Python's >> floors)"""
    return M if t == 0 else (M + (1 << (t - 1))) >> t


def transformed(ch, Mp, L):
    """NTT(Mp mod q_j) for j < L: the rows encrypt_integers hides.  A caller that encrypts one Mp at several L forms the
    rows of the largest once"""
    return [ntt([v % q for v in Mp], ch.psi[j], q) for j, q in enumerate(ch.primes[:L])]


_error_rows = [None, 0, {}]


def encrypt_integers(ch, Mp, L, ek, seed, rows=None):
    """the symmetric encryption [2][L][N] of the integer polynomial Mp: e = sampled_small(ek, 1), c1 from seed;
    rows = transformed(ch, Mp, L' >= L) if the caller has them"""
    N = ch.N
    if _error_rows[:2] != [bytes(ek), N]:   # the rows of the last key stay: one key serves several L
        _error_rows[:] = [bytes(ek), N, {}]
    e = [int(v) for v in sampled_small(bytes(ek), 1, N)]
    rows = transformed(ch, Mp, L) if rows is None else rows
    out = np.empty((2, L, N), dtype=np.uint64)
    for j in range(L):
        q = ch.primes[j]
        if q not in _error_rows[2]:
            _error_rows[2][q] = ntt([v % q for v in e], ch.psi[j], q)
        en = _error_rows[2][q]
        a = expand_limb(bytes(seed), j, q, N)
        out[0][j] = np.array((rows[j] - (_objects(a) * ch.s[j] + en)) % q, dtype=np.uint64)
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
