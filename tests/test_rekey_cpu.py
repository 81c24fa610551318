"""CPU: the contract of re-key to another key pair on the host twin — no GPU.

Key words: rekey_keygen_host equals the Python-integer model of tests/rekey_model.py word for word at N = 1024 under the
chains [60, 30, 45, 50, 33, 60] and [60] * 4 (transforms: the oracle's; one row per chain again through tests/pyref.py's
naive transform).  Key equation: per digit J and row i, c0 + c1 sB - [i == J] P sA has centred coefficients of at most
21 (2 N + 1) — |e| <= 21 (a difference of two 21-bit popcounts), |u| <= 1, |s| <= 1.  Evaluator contract: with that key,
oracle.switch_key((c0, 0), c1, key) at l in {1, 2, k - 1} decrypts under sB to what the input decrypts to under sA, every
slot within rekey_model.slot_bound (inputs in [-1, 1] at scale 2^50).  The randomness contract of make_rekey_key (same
seed, same words; one stream, digits in order, 4 words per digit), the refusals (another N, other primes, no secret key,
size 3) and save / load of a RekeyKey."""
import numpy as np
import pytest

import rekey_model as rm
from eva_amd import _eva
from eva import load, save
from eva.ckks import CKKSParameters
from eva.seal import RekeyKey, SEALValuation, generate_keys
from oracle import pyoracle as po
from sampled_keys import stream_keys

N = 1024
SCALE_BITS = 50
twin = _eva._seal._rekey_keygen_host


class _Pairs:
    """two key pairs over one chain, the re-key key A -> B from the host twin, shared by the tests and never written"""

    def __init__(self, chain):
        self.primes = po.coeff_modulus_create(N, rm.CHAINS[chain])
        self.k, self.D = len(self.primes), len(self.primes) - 1
        self.o = po.Oracle(N, self.primes)
        rng = np.random.default_rng(len(self.primes))
        self.A, self.B = rm.KeyPair(self.o, rng), rm.KeyPair(self.o, rng)
        self.rkeys = np.frombuffer(rng.bytes(32 * self.D), dtype=np.uint8).reshape(self.D, 32)
        self.key = twin(N, self.primes, self.A.s_ntt, self.B.pk, self.rkeys)
        self.rng = rng


@pytest.fixture(scope="module", params=sorted(rm.CHAINS))
def pairs(request):
    return _Pairs(request.param)


def test_key_words_equal_the_integer_model(pairs):
    p = pairs
    assert p.key.shape == (p.D, 2, p.k, N) and p.key.dtype == np.uint64
    model = rm.model_key(p.o, p.B.pk, p.A.s_ntt, p.rkeys)
    assert np.array_equal(p.key, model)
    for i in range(p.k):
        assert int(p.key[:, :, i].max()) < p.primes[i], "canonical residues"
    J = p.D - 1  # one row where the P sA term joins and one where it does not, through pyref's naive transform
    for i in (J, 0):
        d0, d1 = rm.row_by_pyref(p.o, p.B.pk, p.A.s_ntt, p.rkeys[J], J, i)
        assert np.array_equal(d0, p.key[J, 0, i]) and np.array_equal(d1, p.key[J, 1, i]), (J, i)


def test_key_equation(pairs):
    p = pairs
    noise = rm.key_noise(p.o, p.key, p.A.s_ntt, p.B.s_ntt)
    print(f"key noise {noise}, bound {rm.noise_bound(N)}")
    assert 0 < noise <= rm.noise_bound(N)
    # the P sA term is what the bound hangs on: without it the left side is a full-size residue
    assert rm.key_noise(p.o, p.key, np.zeros_like(p.A.s_ntt), p.B.s_ntt) > rm.noise_bound(N)


def _encrypt(p, pair, values, l):
    """(m - (a s + e), a) at l limbs"""
    pt = p.o.encode(l, values, 2.0 ** SCALE_BITS)
    e = p.rng.integers(-rm.ERR_MAX, rm.ERR_MAX + 1, size=N)
    c0, c1 = [], []
    for i in range(l):
        q = p.primes[i]
        a = p.rng.integers(0, q, size=N, dtype=np.uint64)
        b = rm.addmod(rm.mulmod(a, pair.s_ntt[i], q), rm.residues(p.o, i, e), q)
        c0.append(((pt[i].astype(object) - b.astype(object)) % q).astype(np.uint64))
        c1.append(a)
    return np.stack([np.stack(c0), np.stack(c1)])


def test_evaluator_contract(pairs):
    p = pairs
    values = p.rng.uniform(-1, 1, N // 2)
    for l in sorted({1, 2, p.D}):
        ct = _encrypt(p, p.A, values, l)
        under_a = p.o.decode(p.o.decrypt(ct, p.A.s_ntt), 2.0 ** SCALE_BITS)
        ct2 = ct.copy()
        ct2[1] = 0
        out = p.o.switch_key(ct2, np.ascontiguousarray(ct[1]), p.key)
        assert out.shape == ct.shape
        under_b = p.o.decode(p.o.decrypt(out, p.B.s_ntt), 2.0 ** SCALE_BITS)
        diff, bound = float(np.abs(under_b - under_a).max()), rm.slot_bound(N, p.primes, l, SCALE_BITS)
        print(f"l={l}: largest slot difference {diff:.3e}, bound {bound:.3e}; against the values {float(np.abs(under_a - values).max()):.3e}")
        assert diff <= bound
        assert bound < 0.01
        # under the old key the result is noise: the key was switched
        assert float(np.abs(p.o.decode(p.o.decrypt(out, p.A.s_ntt), 2.0 ** SCALE_BITS) - under_a).max()) > 1.0


# ---- the public interface on the host path
@pytest.fixture(scope="module")
def ctxs():
    params = CKKSParameters([60, 30, 45, 50, 33, 60], set(), N)
    return generate_keys(params, 11), generate_keys(params, 12)


def test_make_rekey_key_randomness_contract(ctxs, monkeypatch):
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")  # the host twin, wherever the test runs
    (pub_a, sec_a), (pub_b, sec_b) = ctxs
    rk = sec_a.make_rekey_key(pub_b, seed=5)
    D, k = len(pub_a.primes) - 1, len(pub_a.primes)
    assert isinstance(rk, RekeyKey) and rk.n_digits == D and rk.poly_modulus_degree == N and list(rk.primes) == list(pub_a.primes)
    words = rk.words()
    assert words.shape == (D, 2, k, N)
    assert np.array_equal(sec_a.make_rekey_key(pub_b, seed=5).words(), words), "same seed, same words"
    assert not np.array_equal(sec_a.make_rekey_key(pub_b, seed=6).words(), words)
    assert not np.array_equal(sec_a.make_rekey_key(pub_b).words(), sec_a.make_rekey_key(pub_b).words()), "seed 0: the OS"
    # one secret stream (seed, 3), digit J's key = its words 4 J .. 4 J + 3
    keys = np.frombuffer(b"".join(stream_keys(5, 3, D)), dtype=np.uint8).reshape(D, 32)
    assert np.array_equal(twin(N, list(pub_a.primes), sec_a._secret_key_ntt(), pub_b.public_key(), keys), words)
    assert not np.array_equal(twin(N, list(pub_a.primes), sec_a._secret_key_ntt(), pub_b.public_key(), keys[::-1].copy()), words), "digit order"
    o = po.Oracle(N, list(pub_a.primes))
    assert rm.key_noise(o, words, sec_a._secret_key_ntt(), sec_b._secret_key_ntt()) <= rm.noise_bound(N)


def test_refusals(ctxs, monkeypatch):
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    (pub_a, sec_a), (pub_b, _) = ctxs
    other_n, _ = generate_keys(CKKSParameters([60, 30, 45, 50, 33, 60], set(), 2 * N), 13)
    with pytest.raises(ValueError, match="poly_modulus_degree differs \\(2048 against 1024\\)"):
        sec_a.make_rekey_key(other_n, seed=1)
    other_p, _ = generate_keys(CKKSParameters([60, 30, 45, 50, 34, 60], set(), N), 13)
    with pytest.raises(ValueError, match="prime 4 differs"):
        sec_a.make_rekey_key(other_p, seed=1)
    fewer, _ = generate_keys(CKKSParameters([60, 30, 60], set(), N), 13)
    with pytest.raises(ValueError, match="number of primes differs \\(3 against 6\\)"):
        sec_a.make_rekey_key(fewer, seed=1)
    primes = list(pub_a.primes)
    with pytest.raises(ValueError, match="secret key not present"):
        twin(N, primes, np.zeros((0,), dtype=np.uint64), pub_b.public_key(), np.zeros((5, 32), dtype=np.uint8))
    with pytest.raises(ValueError, match="invalid key digit count"):
        twin(N, primes, sec_a._secret_key_ntt(), pub_b.public_key(), np.zeros((6, 32), dtype=np.uint8))
    rk = sec_a.make_rekey_key(pub_b, seed=1)
    size3 = SEALValuation()
    size3._set_params(pub_a)
    size3._set_cipher("x", np.zeros((3, 2, N), dtype=np.uint64), 2.0 ** 30)
    with pytest.raises(ValueError, match=r"re-key expects a size-2 ciphertext \(relinearize first\)"):
        pub_b.rekey(size3, rk)
    with pytest.raises(ValueError, match="made for other encryption parameters: poly_modulus_degree differs"):
        other_n.install_rekey_key(rk)


def test_save_load_round_trip(ctxs, tmp_path, monkeypatch):
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    (pub_a, sec_a), (pub_b, _) = ctxs
    rk = sec_a.make_rekey_key(pub_b, seed=9)
    path = str(tmp_path / "a_to_b.rekey")
    save(rk, path)
    back = load(path)
    assert isinstance(back, RekeyKey)
    assert back.n_digits == rk.n_digits and back.poly_modulus_degree == N and list(back.primes) == list(rk.primes)
    assert np.array_equal(back.words(), rk.words())
    for fmt in ("seal", "seal+zlib"):
        with pytest.raises(ValueError, match="a RekeyKey has no SEAL format"):
            save(rk, str(tmp_path / "no.seal"), format=fmt)
    raw = bytearray(open(path, "rb").read())
    raw[-8:] = b"\xff" * 8  # a word that is not reduced modulo its prime
    bad = tmp_path / "bad.rekey"
    bad.write_bytes(bytes(raw))
    with pytest.raises(RuntimeError, match="re-key key holds a word that is not reduced"):
        load(str(bad))
