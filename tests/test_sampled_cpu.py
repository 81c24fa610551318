"""CPU: encryption randomness expanded from a 32-byte randomness key per value.  The host twin
sampled_small is compared with a numpy restatement of the rule over the numpy ChaCha20 of test_seeded_cpu.py, its
distribution is checked on 2^20 coefficients of a fixed key, and with EVA_DEVICE_CLIENT=0 encrypt_batch(...,
device_sampling=True) is tied to the host encryptor fed the twin's polynomials."""
import random

import numpy as np
import pytest

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys
from eva_amd import _eva
from oracle import pyoracle as po
from test_seeded_cpu import chacha20

sampled_small = _eva._seal._sampled_small

SAMPLE_TAG = 0x736d000000000000
FIXED_KEY = bytes(range(100, 132))


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    """the host paths on every machine, with or without a GPU (tests/test_gpu_sampled.py covers the device)"""
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


def expand_small(rk, p, N):
    """DESIGN.md 1.7 restated: coefficient j from u64 word j % 8 of block j / 8, nonce SAMPLE_TAG | p"""
    blocks = np.arange((N + 7) // 8, dtype=np.uint64)
    nonce = SAMPLE_TAG | p
    w = chacha20(rk, (blocks & 0xFFFFFFFF).astype(np.uint32), (blocks >> 32).astype(np.uint32),
                 nonce & 0xFFFFFFFF, nonce >> 32).astype(np.uint64)
    w64 = (w[:, 0::2] | (w[:, 1::2] << np.uint64(32))).reshape(-1)[:N]
    if p == 0:
        hi = np.array([(int(x) * 3) >> 64 for x in w64], dtype=np.int64)   # the high word of the 128-bit product
        return (hi - 1).astype(np.int8)
    mask = np.uint64(0x1FFFFF)
    pop = lambda x: np.array([bin(int(v)).count("1") for v in x], dtype=np.int64)
    return (pop(w64 & mask) - pop((w64 >> np.uint64(21)) & mask)).astype(np.int8)


@pytest.mark.parametrize("N", [1024, 4096])
@pytest.mark.parametrize("p", [0, 1, 2])
def test_sampled_small_equals_the_numpy_restatement(N, p):
    for rk in (bytes(32), np.random.default_rng(N + p).integers(0, 256, 32, dtype=np.uint8).tobytes()):
        got = sampled_small(rk, p, N)
        assert got.dtype == np.int8 and got.shape == (N,)
        assert np.array_equal(got, expand_small(rk, p, N)), (N, p, rk.hex())


def test_streams_differ_and_a_shorter_polynomial_is_a_prefix():
    e0, e1 = sampled_small(FIXED_KEY, 1, 4096), sampled_small(FIXED_KEY, 2, 4096)
    assert not np.array_equal(e0, e1)
    assert not np.array_equal(sampled_small(FIXED_KEY, 0, 4096), sampled_small(bytes(32), 0, 4096))
    for p in (0, 1, 2):
        assert np.array_equal(sampled_small(FIXED_KEY, p, 1024), sampled_small(FIXED_KEY, p, 4096)[:1024])
    with pytest.raises(ValueError):
        sampled_small(b"short", 0, 1024)


def test_distribution_of_a_fixed_key():
    n = 1 << 20
    u = sampled_small(FIXED_KEY, 0, n).astype(np.int64)
    assert set(np.unique(u)) == {-1, 0, 1}
    sigma = np.sqrt(n * (1 / 3) * (2 / 3))
    for v in (-1, 0, 1):
        count = int((u == v).sum())
        print(f"ternary {v}: {count} ({(count - n / 3) / sigma:+.2f} sigma)")
        assert abs(count - n / 3) < 5 * sigma, (v, count)
    for p in (1, 2):
        e = sampled_small(FIXED_KEY, p, n).astype(np.float64)
        print(f"error p={p}: max |e| {np.abs(e).max():.0f}, mean {e.mean():+.4f}, variance {e.var(ddof=1):.4f}")
        assert np.abs(e).max() <= 21
        assert abs(e.var(ddof=1) - 10.5) < 0.02 * 10.5   # 42 fair bits: variance 42 / 4


# ---- encrypt_batch(..., device_sampling=True) on the host

def _program(vec_size=512, names=("x", "y")):
    prog = EvaProgram("Sampled", vec_size=vec_size)
    with prog:
        ins = [Input(n) for n in names]
        y = ins[0] * ins[0] + 3 * ins[0]
        for t in ins[1:]:
            y = y + t
        Output("z", y)
    prog.set_output_ranges(20)
    prog.set_input_scales(30)
    return prog


@pytest.fixture(scope="module")
def flow():
    prog = _program()
    _, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    rng = random.Random(3)
    xs = [{n: [rng.uniform(-2, 2) for _ in range(prog.vec_size)] for n in prog.inputs} for _ in range(3)]
    return params, sig, xs


def _words(val, name):
    return np.asarray(val.get(name)[4])


def _stream_keys(seed, stream, n):
    """the first n 32-byte keys of SecureRng(seed, stream): key = seed (8 bytes LE) + the test tag, counter from 0, the
    stream number as the nonce; 4 little-endian words per key = consecutive 32-byte pieces of the output"""
    key = int(seed).to_bytes(8, "little") + b"eva_amd test seed: not secret"[:24]
    blocks = np.arange((n + 1) // 2, dtype=np.uint32)
    out = chacha20(key, blocks, 0, stream & 0xFFFFFFFF, stream >> 32).astype("<u4").tobytes()
    return [out[32 * i: 32 * i + 32] for i in range(n)]


def test_public_encrypt_batch_is_deterministic_and_equals_the_host_encryptor_on_the_twins_polynomials(flow):
    params, sig, xs = flow
    pub, sec = generate_keys(params, 5)
    N = params.poly_modulus_degree
    a = pub.encrypt_batch(xs, sig, device_sampling=True, seed=11)
    b = pub.encrypt_batch(xs, sig, device_sampling=True, seed=11)
    c = pub.encrypt_batch(xs, sig, device_sampling=True, seed=12)
    names = sorted(xs[0])
    keys = _stream_keys(11, 5, len(xs) * len(names))   # instances in list order, names sorted within an instance
    for i, x in enumerate(xs):
        for j, n in enumerate(names):
            assert np.array_equal(_words(a[i], n), _words(b[i], n)), (i, n)
            assert not np.array_equal(_words(a[i], n), _words(c[i], n)), (i, n)
            rk = keys[i * len(names) + j]
            small = np.stack([sampled_small(rk, p, N) for p in range(3)])
            info = sig.inputs[n]
            want = pub._encrypt_with(x[n], info.scale, info.level, small)
            assert np.array_equal(_words(a[i], n), want), f"instance {i}, input {n}"
    got = sec.decrypt_batch(a, sig)
    for i, x in enumerate(xs):
        for n in names:
            assert np.abs(np.array(got[i][n]) - np.array(x[n])).max() < 1e-4, (i, n)
    # OS-keyed streams: two calls differ
    d, e = pub.encrypt_batch(xs, sig, device_sampling=True), pub.encrypt_batch(xs, sig, device_sampling=True)
    assert not np.array_equal(_words(d[0], "x"), _words(e[0], "x"))
    assert np.abs(np.array(sec.decrypt_batch(d, sig)[0]["x"]) - np.array(xs[0]["x"])).max() < 1e-4


def test_a_seed_without_device_sampling_is_refused(flow):
    params, sig, xs = flow
    pub, _ = generate_keys(params, 5)
    with pytest.raises(ValueError, match="device_sampling"):
        pub.encrypt_batch(xs, sig, seed=11)
    with pytest.raises(ValueError, match="device_sampling"):
        pub.encrypt_batch(xs, sig, device_sampling=False, seed=11)
    assert len(pub.encrypt_batch(xs, sig)) == len(xs)


def test_secret_encrypt_batch_keeps_the_seeds_and_takes_the_twins_error(flow):
    params, sig, xs = flow
    pub, sec = generate_keys(params, 5)
    N = params.poly_modulus_degree
    plain = sec.encrypt_batch(xs, sig, seed=9)
    a = sec.encrypt_batch(xs, sig, seed=9, device_sampling=True)
    b = sec.encrypt_batch(xs, sig, seed=9, device_sampling=True)
    names = sorted(xs[0])
    ekeys = _stream_keys(9, 3, len(xs) * len(names))
    sk = sec._secret_key_ntt()
    primes = pub.primes
    oracle = po.Oracle(N, list(primes))
    for i in range(len(xs)):
        for j, n in enumerate(names):
            assert a[i].seed(n) == plain[i].seed(n) and a[i].seed(n) is not None, (i, n)
            wa, wp = _words(a[i], n), _words(plain[i], n)
            assert np.array_equal(wa, _words(b[i], n))
            assert np.array_equal(wa[1], wp[1]) and not np.array_equal(wa[0], wp[0])   # same c1, another error
            # c0 differs from the default call's by NTT(e) - NTT(e'), so c0 + c1 s of both decrypt alike; the error itself:
            # m - (c0 + c1 s) = NTT(e) with e = sampled_small(key, 1), checked on limb 0 through the public encoder
            e = sampled_small(ekeys[i * len(names) + j], 1, N).astype(np.int64)
            q = primes[0]
            info = sig.inputs[n]
            m = pub._encode(xs[i][n], info.scale, info.level)[0].astype(object)
            en = (m - (wa[0][0].astype(object) + wa[1][0].astype(object) * sk[0].astype(object))) % q
            want = oracle.ntt(0, np.array([int(v) % q for v in e], dtype=np.uint64))
            assert np.array_equal(np.array(en, dtype=np.uint64), want), (i, n)
    got = sec.decrypt_batch(a, sig)
    for i, x in enumerate(xs):
        for n in names:
            assert np.abs(np.array(got[i][n]) - np.array(x[n])).max() < 1e-4, (i, n)
