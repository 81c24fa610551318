"""CPU: seed-compressed evaluation keys.  generate_keys(..., compress_keys=True) keeps the
relinearization and Galois keys as c0 plus a 32-byte seed per digit: c1 of every digit is the expansion rule of the
seeded ciphertexts (the numpy restatement of test_seeded_cpu.py) over all k primes, the secret and the public key are
those of the uncompressed key pair, the keys switch correctly (a product and a rotation walked by the CPU oracle), and
the container keeps them compressed while format="seal" writes them expanded."""
import random
import struct

import numpy as np
import pytest

from eva import EvaProgram, Input, Output, evaluate, save, load
from eva.ckks import CKKSCompiler
from eva.metric import valuation_mse
from eva.seal import generate_keys
from evatest import oracle_execute
from test_seeded_cpu import expand_limb

N = 1024


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    """the host encryptor on every machine, with or without a GPU (tests/test_gpu_seeded_keys.py covers the device)"""
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


def _program(vec_size=512):
    prog = EvaProgram("SeededKeys", vec_size=vec_size)
    with prog:
        x = Input("x")
        Output("y", x * x + 3 * x + (x << 1))
    prog.set_output_ranges(20)
    prog.set_input_scales(30)
    return prog


@pytest.fixture(scope="module")
def case():
    prog = _program()
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.poly_modulus_degree = N
    pub, sec = generate_keys(params, 7, compress_keys=True)
    pub0, sec0 = generate_keys(params, 7)
    rng = random.Random(3)
    inputs = {"x": [rng.uniform(-2, 2) for _ in range(prog.vec_size)]}
    return dict(prog=prog, compiled=compiled, params=params, sig=sig, pub=pub, sec=sec, pub0=pub0, sec0=sec0, inputs=inputs)


def _keys(pub):
    """{0: relin words, elt: Galois words} — the materialised [D][2][k][N] arrays"""
    out = {0: pub.relin_key()}
    out.update(pub.galois_keys())
    return out


def test_c1_rows_are_the_expansion_of_their_digit_seed(case):
    pub = case["pub"]
    assert pub.keys_compressed and not case["pub0"].keys_compressed and case["pub0"].key_seeds() is None
    primes, seeds, keys = pub.primes, pub.key_seeds(), _keys(pub)
    k = len(primes)
    assert sorted(seeds) == sorted(keys) and len(keys) >= 2   # the relinearization key and at least one rotation
    all_seeds = set()
    for which, words in keys.items():
        assert words.shape == (k - 1, 2, k, N) and seeds[which].shape == (k - 1, 32) and seeds[which].dtype == np.uint8
        for J in range(k - 1):
            seed = seeds[which][J].tobytes()
            all_seeds.add(seed)
            for i in range(k):   # every chain prime, the special one (i = k - 1) included
                assert np.array_equal(words[J, 1, i], expand_limb(seed, i, primes[i], N)), f"key {which}, digit {J}, row {i}"
                assert int(words[J, 0, i].max()) < primes[i]
    assert len(all_seeds) == len(keys) * (k - 1)   # one seed per digit, none reused


def test_secret_and_public_key_do_not_depend_on_the_option(case):
    assert np.array_equal(case["sec"]._secret_key_ntt(), case["sec0"]._secret_key_ntt())
    assert np.array_equal(case["pub"].public_key(), case["pub0"].public_key())
    assert not np.array_equal(case["pub"].relin_key(), case["pub0"].relin_key())
    g, g0 = case["pub"].galois_keys(), case["pub0"].galois_keys()
    assert sorted(g) == sorted(g0) and all(not np.array_equal(g[e], g0[e]) for e in g)
    # the option is reproducible for one test seed
    again, _ = generate_keys(case["params"], 7, compress_keys=True)
    assert np.array_equal(again.relin_key(), case["pub"].relin_key())


def test_compressed_keys_switch_correctly(case):
    """a product (relinearization) and a rotation walked by the CPU oracle with the materialised keys"""
    pub, sec, sig = case["pub"], case["sec"], case["sig"]
    enc = pub.encrypt(case["inputs"], sig)
    out = oracle_execute(pub, case["compiled"], enc)
    assert valuation_mse(sec.decrypt(out, sig), evaluate(case["prog"], case["inputs"])) < 0.01


def test_save_load_keeps_the_keys_compressed(case, tmp_path):
    pub, pub0 = case["pub"], case["pub0"]
    fc, ff = tmp_path / "c.sealpub", tmp_path / "f.sealpub"
    save(pub, str(fc))
    save(pub0, str(ff))
    back = load(str(fc))
    assert back.keys_compressed and back.primes == pub.primes
    s0, s1 = pub.key_seeds(), back.key_seeds()
    assert sorted(s0) == sorted(s1) and all(np.array_equal(s0[e], s1[e]) for e in s0)
    k0, k1 = _keys(pub), _keys(back)
    for e in k0:
        assert np.array_equal(k0[e][:, 0], k1[e][:, 0]), f"c0 of key {e}"
        assert np.array_equal(k0[e], k1[e]), f"materialised words of key {e}"
    assert np.array_equal(back.public_key(), pub.public_key())
    # the bound follows from the two layouts: a key is D (2 k N) words in full and D (k N) words + 32 D bytes compressed,
    # the public key and the headers are written alike
    k, D, n_keys = len(pub.primes), len(pub.primes) - 1, len(k0)
    pk_bytes = 2 * k * N * 8
    assert fc.stat().st_size <= ff.stat().st_size / 2 + pk_bytes / 2 + 32 * D * n_keys + 256, (fc.stat().st_size, ff.stat().st_size)
    # an uncompressed context is written as before: the same bytes for the same key pair, and it loads uncompressed
    again, _ = generate_keys(case["params"], 7)
    save(again, str(tmp_path / "f2.sealpub"))
    assert (tmp_path / "f2.sealpub").read_bytes() == ff.read_bytes()
    full = load(str(ff))
    assert not full.keys_compressed and np.array_equal(full.relin_key(), pub0.relin_key())


def test_uncompressed_file_layout_is_the_parents(case, tmp_path):
    """the container of an uncompressed context, restated field by field: N, primes, public key, then per key the
    plain digit count and the full words — no flag, no seeds"""
    pub0 = case["pub0"]
    path = tmp_path / "f.sealpub"
    save(pub0, str(path))
    primes = pub0.primes
    k = len(primes)
    want = struct.pack("<III", 0x48415645, 1, 5) + struct.pack("<I", N) + struct.pack("<Q", k) + np.array(primes, dtype="<u8").tobytes()
    want += struct.pack("<Q", 2 * k * N) + pub0.public_key().astype("<u8").tobytes()
    rk = pub0.relin_key()
    want += struct.pack("<IQ", rk.shape[0], rk.size) + rk.astype("<u8").tobytes()
    gk = pub0.galois_keys()
    want += struct.pack("<Q", len(gk))
    for elt in sorted(gk):
        want += struct.pack("<IIQ", elt, gk[elt].shape[0], gk[elt].size) + gk[elt].astype("<u8").tobytes()
    assert path.read_bytes() == want


@pytest.mark.parametrize("fmt", ["seal", "seal+zlib"])
def test_seal_format_writes_the_materialised_keys(case, tmp_path, fmt):
    pub = case["pub"]
    path = str(tmp_path / "c.seal")
    save(pub, path, format=fmt)
    back = load(path)
    assert not back.keys_compressed and back.key_seeds() is None
    k0, k1 = _keys(pub), _keys(back)
    assert sorted(k0) == sorted(k1) and all(np.array_equal(k0[e], k1[e]) for e in k0)
    assert np.array_equal(back.public_key(), pub.public_key())


def test_hostile_compressed_files_are_rejected(case, tmp_path):
    pub, pub0 = case["pub"], case["pub0"]
    path = tmp_path / "c.sealpub"
    save(pub, str(path))
    raw = path.read_bytes()
    primes = pub.primes
    k, D = len(primes), len(primes) - 1
    # the relinearization key follows the header (12), N (4), the primes (8 + 8 k) and the public key (8 + 16 k N):
    # flagged digit count, seed bytes (length, data), c0 (length, words)
    at = 12 + 4 + 8 + 8 * k + 8 + 16 * k * N
    assert struct.unpack_from("<IQ", raw, at) == (D | 0x80000000, 32 * D)
    seeds_at = at + 4 + 8
    c0_len_at = seeds_at + 32 * D
    assert struct.unpack_from("<Q", raw, c0_len_at)[0] == D * k * N
    bad = tmp_path / "bad.sealpub"

    # a seed array one byte short
    bad.write_bytes(raw[:at + 4] + struct.pack("<Q", 32 * D - 1) + raw[seeds_at:c0_len_at - 1] + raw[c0_len_at:])
    with pytest.raises(RuntimeError, match="wrong size|parse"):
        load(str(bad))
    # a c0 word >= its prime (row 0 of digit 0: prime 0)
    w = bytearray(raw)
    struct.pack_into("<Q", w, c0_len_at + 8 + 8 * 5, primes[0])
    bad.write_bytes(bytes(w))
    with pytest.raises(RuntimeError, match="not reduced"):
        load(str(bad))
    # the flag set in front of a full-size payload
    full = tmp_path / "f.sealpub"
    save(pub0, str(full))
    w = bytearray(full.read_bytes())
    assert struct.unpack_from("<I", w, at)[0] == D
    struct.pack_into("<I", w, at, D | 0x80000000)
    bad.write_bytes(bytes(w))
    with pytest.raises(RuntimeError, match="wrong size|parse"):
        load(str(bad))
    # and the untouched file still loads
    assert load(str(path)).keys_compressed
