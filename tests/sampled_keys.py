"""What the tests of the sampled key set share: the shapes, the derivation of the two test streams restated
in numpy, and the key equation in Python integers for a whole key pair.  No test of its own."""
import struct

import numpy as np

from eva_amd import _eva
from eva.ckks import CKKSParameters
from oracle import pyoracle as po
from test_seeded_cpu import chacha20, expand_limb

sampled_small = _eva._seal._sampled_small

# tests/test_gpu_keygen.py's: the smallest shapes that reach every branch of the kernel and its launch
SHAPES = {
    "N1024_mixed": (1024, [60, 30, 45, 50, 33, 60], (1, -3, 0)),   # mixed prime sizes, a split copy; step 0 = conjugation (2N - 1)
    "N2048_topbit": (2048, [60, 50, 50, 60], (5,)),                # all top-bit, blockIdx.x > 0
    "N1024_17digits": (1024, [30] * 16 + [31, 31], (2,)),          # 17 digits: grid.z far above 8
}


def params_of(name):
    N, bits, steps = SHAPES[name]
    return CKKSParameters(list(bits), set(steps), N)


def keys_of(pub):
    """{0: relin words, elt: Galois words} — the materialised [D][2][k][N] arrays"""
    out = {0: pub.relin_key()}
    out.update(pub.galois_keys())
    return out


def elt_of_step(N, step):
    return 2 * N - 1 if step == 0 else po.galois_elt_from_step(N, step)


def key_order(name):
    """the keys of a shape in generate_keys' order: 0 (relinearization), then the Galois elements in the order of
    params.rotations — a sorted set of steps"""
    N, _, steps = SHAPES[name]
    return [0] + [elt_of_step(N, st) for st in sorted(set(steps))]


def stream_keys(seed, stream, n):
    """the first n 32-byte keys of SecureRng(seed, stream) (csprng.h): ChaCha20 keyed with the 8 seed bytes and a fixed
    tag, the stream number as the nonce, block counter from 0 — 64 bytes per block, 4 generator words per key"""
    key = struct.pack("<Q", seed) + b"eva_amd test seed: not secret"[:24]
    blocks = np.arange((n + 1) // 2, dtype=np.uint32)
    raw = chacha20(key, blocks, 0, stream & 0xFFFFFFFF, stream >> 32).astype("<u4").tobytes()
    return [raw[32 * i:32 * i + 32] for i in range(n)]


def automorphism(s, elt, N):
    """coefficients of s(X^elt) in Z[X] / (X^N + 1)"""
    out = np.zeros(N, dtype=np.int64)
    for j in range(N):
        m = (j * elt) % (2 * N)
        if m < N:
            out[m] += s[j]
        else:
            out[m - N] -= s[j]
    return out


def _residues(o, i, small):
    q = o.primes[i]
    return o.ntt(i, np.array([int(v) % q for v in small], dtype=np.uint64))


def check_key_pair(pub, sec, rand):
    """the whole contract of DESIGN.md 1.8 for one key pair, in Python integers and without the host generator: s is
    sampled_small(rk_s, 0); the public key and every digit and prime of every evaluation key satisfy the key equation with
    c1 the expansion of the key's seed, and the error recovered from it is exactly sampled_small(its key, 1)"""
    N, primes = pub.poly_modulus_degree, pub.primes
    k, D = len(primes), len(primes) - 1
    o = po.Oracle(N, primes)
    P = primes[-1]
    s = sampled_small(rand["secret"], 0, N)
    assert set(np.unique(s)) <= {-1, 0, 1}
    s_ntt = np.stack([_residues(o, i, s) for i in range(k)])
    assert np.array_equal(sec._secret_key_ntt(), s_ntt), "s = sampled_small(rk_s, 0)"

    def error_of(c0_row, c1_row, i, extra):
        q = primes[i]
        m = [(int(b) + int(a) * int(sv) - x) % q for b, a, sv, x in zip(c0_row, c1_row, s_ntt[i], extra)]
        return o.intt(i, np.array(m, dtype=np.uint64))

    def minus(e, q):
        return np.array([(-int(v)) % q for v in e], dtype=np.uint64)
    pk = pub.public_key()
    e_pk = sampled_small(rand["public"], 1, N)
    for i, q in enumerate(primes):
        assert np.array_equal(error_of(pk[0, i], pk[1, i], i, [0] * N), minus(e_pk, q)), f"public key, prime {i}"
    seeds, words = pub.key_seeds(), keys_of(pub)
    assert sorted(seeds) == sorted(words) == sorted(e for e in rand if isinstance(e, int))
    for elt, w in words.items():
        assert w.shape == (D, 2, k, N) and rand[elt].shape == (D, 32) and seeds[elt].shape == (D, 32)
        sp = None if elt == 0 else automorphism(s, elt, N)
        errors = [sampled_small(rand[elt][J].tobytes(), 1, N) for J in range(D)]
        for i, q in enumerate(primes):
            if elt == 0:
                spi = [int(v) * int(v) % q for v in s_ntt[i]]
            else:
                spi = [int(v) for v in _residues(o, i, sp)]
            for J in range(D):
                assert np.array_equal(w[J, 1, i], expand_limb(seeds[elt][J].tobytes(), i, q, N)), f"key {elt}, digit {J}, prime {i}: c1"
                f = P % q if i == J else 0
                got = error_of(w[J, 0, i], w[J, 1, i], i, [f * v for v in spi])
                assert np.array_equal(got, minus(errors[J], q)), f"key {elt}, digit {J}, prime {i}"
