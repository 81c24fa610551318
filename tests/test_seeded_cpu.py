"""CPU: secret-key encryption with seed-compressed ciphertexts.  The expansion of c1 = a from its
32-byte seed is re-derived here with a numpy ChaCha20 (checked against RFC 8439) and compared with the host's; the
host secret_ctx.encrypt round-trips through decrypt, save / load and the SEAL format, and a compiled program walked
over the CPU oracle gives the same words on seeded inputs as on their materialised copies."""
import random

import numpy as np
import pytest

from eva import EvaProgram, Input, Output, evaluate, save, load
from eva.ckks import CKKSCompiler
from eva.metric import valuation_mse
from eva.seal import generate_keys, SEALValuation
from evatest import oracle_execute


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    """the host encryptor on every machine, with or without a GPU (tests/test_gpu_seeded.py covers the device one)"""
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


SIGMA = np.array([0x61707865, 0x3320646e, 0x79622d32, 0x6b206574], dtype=np.uint32)
NONCE_TAG = 0x6331000000000000


def _rotl(x, r):
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def chacha20(key, w12, w13, w14, w15):
    """RFC 8439 block function, vectorised over the blocks: key 32 bytes, state words 12-15 as arrays -> [n][16]"""
    w12 = np.atleast_1d(np.asarray(w12, dtype=np.uint32))
    n = w12.shape[0]
    kw = np.frombuffer(bytes(key), dtype="<u4")
    init = np.empty((16, n), dtype=np.uint32)
    init[0:4] = SIGMA[:, None]
    init[4:12] = kw[:, None]
    init[12] = w12
    init[13] = np.broadcast_to(np.asarray(w13, dtype=np.uint32), (n,))
    init[14] = np.broadcast_to(np.asarray(w14, dtype=np.uint32), (n,))
    init[15] = np.broadcast_to(np.asarray(w15, dtype=np.uint32), (n,))
    x = [init[i].copy() for i in range(16)]

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = _rotl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        out = np.stack(x) + init
    return out.T


def expand_limb(seed, i, q, N):
    """limb i of a: coefficient j = (hi 2^64 + lo) mod q, (lo, hi) = u64 words 2 (j % 4), 2 (j % 4) + 1 of block j / 4"""
    blocks = np.arange(N // 4, dtype=np.uint64)
    nonce = NONCE_TAG | i
    w = chacha20(seed, (blocks & 0xFFFFFFFF).astype(np.uint32), (blocks >> 32).astype(np.uint32),
                 nonce & 0xFFFFFFFF, nonce >> 32).astype(np.uint64)
    w64 = (w[:, 0::2] | (w[:, 1::2] << np.uint64(32))).reshape(N // 4, 4, 2)   # [block][coefficient][lo, hi]
    lo, hi = w64[..., 0].reshape(N), w64[..., 1].reshape(N)
    two64 = pow(2, 64, q)
    v = (hi.astype(object) % q * two64 + lo.astype(object)) % q
    return np.array(v, dtype=np.uint64)


def test_rfc8439_block_vector():
    """RFC 8439 section 2.3.2: key 00..1f, block count 1, nonce 00:00:00:09:00:00:00:4a:00:00:00:00"""
    key = bytes(range(32))
    out = chacha20(key, 1, 0x09000000, 0x4a000000, 0)[0]
    want = bytes.fromhex(
        "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
        "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert out.astype("<u4").tobytes() == want


def _program(vec_size=512, names=("x",)):
    prog = EvaProgram("Seeded", vec_size=vec_size)
    with prog:
        ins = [Input(n) for n in names]
        y = ins[0] * ins[0] + 3 * ins[0]
        for t in ins[1:]:
            y = y + t
        Output("y", y)
    prog.set_output_ranges(20)
    prog.set_input_scales(30)
    return prog


def _compile(prog, N=None, bits=None):
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    if N is not None:
        params.poly_modulus_degree = N
    if bits is not None:
        params.prime_bits = list(bits)
    return compiled, params, sig


def _inputs(prog, seed=3):
    rng = random.Random(seed)
    return {n: [rng.uniform(-2, 2) for _ in range(prog.vec_size)] for n in prog.inputs}


def _check_expansion(N, bits, vec_size):
    prog = _program(vec_size, ("a", "b"))
    _, params, sig = _compile(prog, N, bits)
    pub, sec = generate_keys(params, 9)
    enc = sec.encrypt(_inputs(prog), sig, seed=21)
    primes = pub.primes
    for name in enc.names():
        seed = enc.seed(name)
        assert isinstance(seed, bytes) and len(seed) == 32
        kind, size, limbs, _, data = enc.get(name)
        assert kind == "cipher" and size == 2 and limbs == len(primes) - 1 - sig.inputs[name].level
        for i in range(limbs):
            assert np.array_equal(data[1][i], expand_limb(seed, i, primes[i], N)), f"{name}: limb {i} of c1"
            assert int(data[0][i].max()) < primes[i]


def test_expansion_matches_host_mixed_primes():
    _check_expansion(1024, [60, 30, 45, 50, 33, 60], 512)


def test_expansion_matches_host_2_16_all_limbs():
    _check_expansion(1 << 16, [60] + [50] * 9 + [60], 512)


def test_round_trip_decrypt():
    prog = _program()
    _, params, sig = _compile(prog)
    pub, sec = generate_keys(params, 5)
    inputs = _inputs(prog)
    enc = sec.encrypt(inputs, sig)
    assert valuation_mse(sec.decrypt(enc, sig), inputs) < 0.01
    assert enc.on_host("x") and not enc.is_resident("x")


def test_same_seed_same_valuation_distinct_seeds():
    prog = _program(names=("a", "b", "c"))
    _, params, sig = _compile(prog)
    pub, sec = generate_keys(params, 5)
    inputs = _inputs(prog)
    e1, e2 = sec.encrypt(inputs, sig, seed=77), sec.encrypt(inputs, sig, seed=77)
    for n in inputs:
        assert e1.seed(n) == e2.seed(n)
        assert np.array_equal(e1.get(n)[4], e2.get(n)[4])
    assert len({e1.seed(n) for n in inputs}) == len(inputs)
    e3 = sec.encrypt(inputs, sig, seed=78)
    assert all(e3.seed(n) != e1.seed(n) for n in inputs)
    e4, e5 = sec.encrypt(inputs, sig), sec.encrypt(inputs, sig)   # OS-keyed streams
    assert all(e4.seed(n) != e5.seed(n) for n in inputs)
    # public-key ciphertexts and values that never went through encrypt carry no seed
    assert pub.encrypt(inputs, sig).seed("a") is None


def test_save_load_and_size(tmp_path):
    prog = _program(names=("a", "b"))
    _, params, sig = _compile(prog)
    pub, sec = generate_keys(params, 5)
    inputs = _inputs(prog)
    enc = sec.encrypt(inputs, sig, seed=4)
    save(enc, str(tmp_path / "s.sealvals"))
    back = load(str(tmp_path / "s.sealvals"))
    for n in inputs:
        assert back.seed(n) == enc.seed(n)
        a, b = enc.get(n), back.get(n)
        assert a[:4] == b[:4] and np.array_equal(a[4], b[4])
    assert valuation_mse(sec.decrypt(back, sig), inputs) < 0.01
    save(pub.encrypt(inputs, sig), str(tmp_path / "p.sealvals"))
    seeded_bytes = (tmp_path / "s.sealvals").stat().st_size
    full_bytes = (tmp_path / "p.sealvals").stat().st_size
    assert seeded_bytes <= 0.55 * full_bytes, (seeded_bytes, full_bytes)


def test_seal_format_writes_the_expanded_ciphertext(tmp_path):
    prog = _program(names=("a", "b"))
    _, params, sig = _compile(prog)
    pub, sec = generate_keys(params, 5)
    enc = sec.encrypt(_inputs(prog), sig, seed=6)
    mat = SEALValuation()
    for n in enc.names():
        _, _, _, scale, data = enc.get(n)
        mat._set_cipher(n, data, scale)
    mat._set_params(pub)
    save(enc, str(tmp_path / "s.seal"), format="seal")
    save(mat, str(tmp_path / "m.seal"), format="seal")
    assert (tmp_path / "s.seal").read_bytes() == (tmp_path / "m.seal").read_bytes()


def test_oracle_walk_on_seeded_inputs():
    prog = _program(names=("a", "b"))
    compiled, params, sig = _compile(prog)
    pub, sec = generate_keys(params, 5)
    inputs = _inputs(prog)
    enc = sec.encrypt(inputs, sig, seed=8)
    mat = SEALValuation()
    for n in enc.names():
        _, _, _, scale, data = enc.get(n)
        mat._set_cipher(n, data, scale)
    fresh = sec.encrypt(inputs, sig, seed=8)   # not materialised by get() before the walk
    out_s, out_m = oracle_execute(pub, compiled, fresh), oracle_execute(pub, compiled, mat)
    for n in out_m.names():
        assert np.array_equal(out_s.get(n)[4], out_m.get(n)[4])
    assert valuation_mse(sec.decrypt(out_s, sig), evaluate(prog, inputs)) < 0.01
