"""CPU: the refresh on the host twin against a Python-integer model of its contract, word for word, on short
chains and at the levels of long ones where the device kernel changes its form; what the device test's edge lists reach
(tests/refresh_edges.py); its refusals, its randomness contract and the file format of its results."""
import numpy as np
import pytest

import refresh_edges as edges
import refresh_model as rm
from eva import save, load
from eva.ckks import CKKSParameters, CKKSSignature, CKKSEncodingInfo
from eva.seal import generate_keys, SEALValuation
from eva_amd._eva import Type
from eva_amd.hostref import coeff_modulus_create
from pyref import centered, crt, naive_ntt
from sampled_keys import stream_keys

N = 1024
CHAINS = edges.CHAINS
B_BITS = 20   # the target scale 2^b


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    """the host twin on every machine (tests/test_gpu_refresh.py covers the device)"""
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


_cache = {}


def keys(chain):
    if chain not in _cache:
        pub, sec = generate_keys(CKKSParameters(list(CHAINS[chain]), set(), N), 11)
        _cache[chain] = (pub, sec, rm.Chain(N, pub.primes, sec._secret_key_ntt()))
    return _cache[chain]


def signature(k, L, names=("x",), scale=B_BITS):
    return CKKSSignature(64, {n: CKKSEncodingInfo(Type.Cipher, scale, k - 1 - L) for n in names})


def valuation(name, ct, a_bits):
    v = SEALValuation()
    v._set_cipher(name, ct, 2.0 ** a_bits)
    return v


def random_ct(primes, size, l, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.integers(0, primes[i], size=N, dtype=np.uint64) for i in range(l)]) for _ in range(size)])


def test_model_transform_is_the_naive_one():
    q = keys("mixed")[2].primes[1]
    psi = rm.minimal_psi(256, q)
    a = [int(v) for v in np.random.default_rng(1).integers(0, q, size=256)]
    assert [int(v) for v in rm.ntt(a, psi, q)] == naive_ntt(a, psi, q)
    assert [int(v) for v in rm.intt(rm.ntt(a, psi, q), psi, q)] == a


def test_model_recomposition_is_pyref_crt():
    primes = keys("mixed")[2].primes[:5]
    rows = [rm._objects(np.random.default_rng(i).integers(0, q, size=8)) for i, q in enumerate(primes)]
    want = [centered(*crt([int(r[n]) for r in rows], primes)) for n in range(8)]
    assert rm.crt_centered(rows, primes) == want and max(want) > 0 > min(want)


def _levels(chain):
    k = len(CHAINS[chain])
    return [(1, k - 1), (2, k - 1), (k - 1, k - 1), (3, 2)]


@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("case", [(c, i) for c in ("mixed", "all60") for i in range(4)], ids=lambda c: f"{c[0]}-{c[1]}")
def test_host_twin_equals_model(case, size):
    chain, idx = case
    pub, sec, ch = keys(chain)
    l, L = _levels(chain)[idx]
    k = len(ch.primes)
    ct = random_ct(ch.primes, size, l, 100 * idx + size)
    M = rm.decrypt_integers(ch, ct)
    assert max(M) > 0 > min(M)
    for t in (0, 1, 30, 62):
        seed = 1000 + t
        got = sec.refresh(valuation("x", ct, B_BITS + t), signature(k, L), seed=seed)
        kind, gsize, limbs, scale, words = got.get("x")
        assert (kind, gsize, limbs, scale) == ("cipher", 2, L, 2.0 ** B_BITS)
        want = rm.refresh(ch, ct, L, t, stream_keys(seed, 3, 1)[0], stream_keys(seed, 4, 1)[0], M=M)
        assert np.array_equal(words, want), (chain, l, L, t, size)


@pytest.mark.parametrize("case", edges.FORM_CASES, ids=edges.form_case_id)
def test_edge_list_reaches_every_reachable_branch(case):
    """the lists test_gpu_refresh.py refreshes at every (chain, l, t) of its kernel-form test, accounted for in Python
    integers: every branch the triple allows is taken, the sign decision at every digit position in both directions
    among them, and every branch it does not allow is named here with its reason"""
    chain, l, ts = case
    primes = coeff_modulus_create(N, CHAINS[chain])
    k = len(primes)
    for t in ts:
        M = edges.form_messages(primes, l, t)
        assert len(M) == N
        hit = edges.coverage(primes, l, t, M)
        yes, no = edges.reachable(primes, l, t)
        assert not set(no) & yes
        assert hit == yes, (chain, l, t, "missed", sorted(yes - hit), "beyond reachable", sorted(hit - yes))
        assert {f"sign_{s}_at_{i}" for i in range(l) for s in ("neg", "pos")} <= hit
        # what is out of reach, spelled out: the chains of one width list their primes in ascending order, so no digit
        # reaches a later prime; on the mixed chain only l = k - 1 leaves no prime to lift to; t = 0 forms no remainder,
        # t = 1 has d in {0, 1}, and 2^(t-1) reaches a 60-bit prime at t = 62 only, a 30-bit one from t = 31 on
        want_no = set()
        if chain in ("w60x21", "b30x62"):
            want_no |= {"digit_over_in_garner", "digit_over_in_lift"}
        elif l == k - 1:
            want_no |= {"digit_over_in_lift"}
        if t == 0:
            want_no |= {"d_neg", "d_zero", "d_pos", "d_top", "d_over_prime_neg", "d_over_prime_pos"}
        if t == 1:
            want_no |= {"d_neg", "d_pos", "d_over_prime_neg", "d_over_prime_pos"}
        if t == 31 and chain == "w60x21":
            want_no |= {"d_over_prime_neg", "d_over_prime_pos"}
        assert set(no) == want_no, (chain, l, t, no)


LONG_CASES = [(c, l) for c in ("w60x21", "mixed21") for l in (4, 8, 9, 16, 17)] + [("b30x62", 61)]
SIZE_AT = {4: 1, 8: 2, 9: 3, 16: 2, 17: 3, 61: 2}   # sizes 1 and 3 ride along: the dot product's powers of the key


@pytest.mark.parametrize("case", LONG_CASES, ids=lambda c: f"{c[0]}-l{c[1]}")
def test_host_twin_equals_model_on_long_chains(case):
    """refresh_lift_coeff at the levels where the device kernel changes its form (4 | 5, 8 | 9, 16 | 17) and at the
    deepest level there is, to fewer, as many and more primes than the value has, at both ends of the shift"""
    chain, l = case
    pub, sec, ch = keys(chain)
    k, size = len(ch.primes), SIZE_AT[l]
    ct = random_ct(ch.primes, size, l, 31 * l + size)
    M = rm.decrypt_integers(ch, ct)
    assert max(M) > 0 > min(M)
    Ls = sorted({L for L in (1, l - 1, l, l + 1, k - 1) if 1 <= L <= k - 1})
    assert Ls[0] < l and l in Ls and (Ls[-1] > l or l == k - 1)
    for t in (0, 62):
        seed = 1000 + t
        ek, sd = stream_keys(seed, 3, 1)[0], stream_keys(seed, 4, 1)[0]
        rows = rm.transformed(ch, [rm.divide(v, t) for v in M], Ls[-1])
        for L in Ls:
            kind, gsize, limbs, scale, words = sec.refresh(valuation("x", ct, B_BITS + t), signature(k, L), seed=seed).get("x")
            assert (kind, gsize, limbs, scale) == ("cipher", 2, L, 2.0 ** B_BITS)
            bad = np.argwhere(words != rm.encrypt_integers(ch, None, L, ek, sd, rows=rows))
            assert bad.size == 0, (chain, l, L, t, "first differing (poly, limb, n)", bad[0], "M", M[bad[0][2]])


@pytest.mark.parametrize("case", [("mixed21", 4), ("mixed21", 17), ("w60x21", 9)], ids=lambda c: f"{c[0]}-l{c[1]}")
def test_host_twin_at_every_digit_position(case):
    """the edge list of the device test through the host twin: the sign decided at every digit, both ways"""
    chain, l = case
    pub, sec, ch = keys(chain)
    k, t, L = len(ch.primes), 31, len(ch.primes) - 1
    M = edges.form_messages(ch.primes, l, t)
    ct = rm.message_ciphertext(ch, M, l)
    words = sec.refresh(valuation("x", ct, B_BITS + t), signature(k, L), seed=6).get("x")[4]
    bad = np.argwhere(words != rm.encrypt_integers(ch, [rm.divide(v, t) for v in M], L, stream_keys(6, 3, 1)[0], stream_keys(6, 4, 1)[0]))
    assert bad.size == 0, (chain, l, "first differing (poly, limb, n)", bad[0], "M", M[bad[0][2]])


def test_ties_round_towards_plus_infinity():
    """M = +-(2^(t-1)) mod 2^t and their neighbours, both signs, through the host twin"""
    pub, sec, ch = keys("mixed")
    l, L, t, k = 2, 5, 4, 6
    M = [0] * N
    edge = [8, -8, 24, -24, 7, 9, -7, -9, 23, 25, -23, -25, 1, -1]
    M[:len(edge)] = edge
    assert [rm.divide(v, t) for v in edge[:4]] == [1, 0, 2, -1]   # never "to nearest even", never "away from zero"
    ct = rm.message_ciphertext(ch, M, l)
    assert rm.decrypt_integers(ch, ct) == M
    got = sec.refresh(valuation("x", ct, B_BITS + t), signature(k, L), seed=5).get("x")[4]
    assert np.array_equal(got, rm.refresh(ch, ct, L, t, stream_keys(5, 3, 1)[0], stream_keys(5, 4, 1)[0]))


def test_refusals():
    pub, sec, ch = keys("all60")
    k = 4
    ct = random_ct(ch.primes, 2, 2, 3)
    sig = signature(k, 3)
    errors = (ValueError, RuntimeError, IndexError, KeyError)
    with pytest.raises(errors, match="power of two"):
        v = SEALValuation()
        v._set_cipher("x", ct, 3.0 * 2.0 ** 20)
        sec.refresh(v, sig)
    with pytest.raises(errors, match="target scale is above"):
        sec.refresh(valuation("x", ct, B_BITS - 1), sig)
    with pytest.raises(errors, match="exceeds 2\\^62"):
        sec.refresh(valuation("x", ct, B_BITS + 64), sig)
    with pytest.raises(errors, match="exceeds 2\\^62"):
        sec.refresh(valuation("x", ct, B_BITS + 63), sig)
    with pytest.raises(errors, match="nowhere"):
        sec.refresh(valuation("x", ct, B_BITS), sig, rename={"x": "nowhere"})
    with pytest.raises(errors, match="No input named"):
        sec.refresh(valuation("x", ct, B_BITS), sig, inputs={"w": [0.0] * 64})
    with pytest.raises(errors, match="exceeds the modulus chain"):
        sec.refresh(valuation("x", ct, B_BITS), signature(k, 0))
    # the source may be renamed, and the consumer's unencrypted inputs ride along
    sig2 = CKKSSignature(64, {"x": CKKSEncodingInfo(Type.Cipher, B_BITS, 0), "w": CKKSEncodingInfo(Type.Raw, B_BITS, 0)})
    out = sec.refresh(valuation("y", ct, B_BITS), sig2, rename={"x": "y"}, inputs={"w": [1.5] * 64})
    assert sorted(out.names()) == ["w", "x"] and out.get("w")[0] == "raw" and out.get("w")[4] == [1.5] * 64


def test_randomness_contract():
    pub, sec, ch = keys("all60")
    k, seed = 4, 77
    ct = random_ct(ch.primes, 2, 3, 9)
    one = sec.refresh(valuation("x", ct, B_BITS), signature(k, 3), seed=seed)
    assert one.seed("x") == stream_keys(seed, 4, 1)[0]
    assert np.array_equal(one.get("x")[4], rm.refresh(ch, ct, 3, 0, stream_keys(seed, 3, 1)[0], stream_keys(seed, 4, 1)[0]))
    # two values of one call: names sorted, consecutive keys of both streams, never a shared seed
    v = SEALValuation()
    v._set_cipher("b", ct, 2.0 ** B_BITS)
    v._set_cipher("a", random_ct(ch.primes, 2, 3, 10), 2.0 ** B_BITS)
    two = sec.refresh(v, signature(k, 3, names=("a", "b")), seed=seed)
    sd, ek = stream_keys(seed, 4, 2), stream_keys(seed, 3, 2)
    assert [two.seed("a"), two.seed("b")] == sd and sd[0] != sd[1]
    assert np.array_equal(two.get("b")[4], rm.refresh(ch, ct, 3, 0, ek[1], sd[1]))
    # OS-keyed streams: no two calls share a seed
    assert sec.refresh(v, signature(k, 3, names=("a", "b"))).seed("a") != sec.refresh(v, signature(k, 3, names=("a", "b"))).seed("a")


def test_saves_as_a_seeded_value(tmp_path):
    pub, sec, ch = keys("all60")
    ct = random_ct(ch.primes, 2, 2, 4)
    out = sec.refresh(valuation("x", ct, B_BITS + 1), signature(4, 3), seed=8)
    full = SEALValuation()
    full._set_cipher("x", out.get("x")[4], 2.0 ** B_BITS)
    save(out, str(tmp_path / "r.sealvals"))
    save(full, str(tmp_path / "f.sealvals"))
    back = load(str(tmp_path / "r.sealvals"))
    assert back.seed("x") == out.seed("x") == stream_keys(8, 4, 1)[0]
    a, b = out.get("x"), back.get("x")
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4])
    # value kind 4 (c0 + seed): about half the bytes of the same words written in full
    assert (tmp_path / "r.sealvals").stat().st_size <= 0.55 * (tmp_path / "f.sealvals").stat().st_size
