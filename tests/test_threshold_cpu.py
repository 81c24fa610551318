"""CPU: the contract of threshold decryption on the host twins — no GPU.

Flooding noise: _flood_wide equals the numpy-ChaCha20 restatement of tests/threshold_model.py at sigma in {1, 21, 40, 62},
stays in [-2^sigma, 2^sigma), a shorter N is a prefix, the nonce tag is its own.  Collective keys: three
generate_keys(seed=s_p, common_seed=c) pairs share pk[1] and every seed, differ in their secrets, and each is a valid key
pair alone; combine_public_contexts satisfies the key equations under s = sum_p s_p in integers (public key and every
Galois digit centred within 21 P: each party's error is a difference of two 21-bit popcounts), and refuses a foreign seed
and other primes.  Host share and combine: the share's words equal the model, m equals (c0 + c1 s + sum_p NTT(E_p)) mod q
word for word at l in {1, 2, k - 1} and P in {1, 2, 3}, the doubles equal the oracle's decode of m bit for bit, a slot
differs from the plain decryption under s by at most N P 2^sigma / scale, and the room refusals fire exactly at their
thresholds.  N = 1024 on [60, 30, 45, 50, 33, 60] and [60] * 4."""
import numpy as np
import pytest

import threshold_model as tm
from eva import load, save
from eva.ckks import CKKSParameters
from eva.seal import SEALPublic, combine_public_contexts, generate_keys
from eva_amd import _eva
from oracle import pyoracle as po
from pyref import centered
from refresh_model import Chain, ntt
from sampled_keys import automorphism

N = 1024
CHAINS = {"mixed": [60, 30, 45, 50, 33, 60], "all60": [60] * 4}
flood_wide = _eva._seal._flood_wide
share_host = _eva._seal._decrypt_share_host
combine_host = _eva._seal._combine_shares_host
COMMON = bytes(range(7, 39))


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


def fkey(i):
    return bytes((i * 29 + j * 13 + 3) % 256 for j in range(32))


# ---- the flooding noise
@pytest.mark.parametrize("sigma", [1, 21, 40, 62])
def test_flood_wide_equals_the_model(sigma):
    for fk in (bytes(32), fkey(sigma)):
        got = flood_wide(fk, sigma, N)
        assert got.dtype == np.int64 and got.shape == (N,)
        assert [int(v) for v in got] == tm.flood(fk, sigma, N), (sigma, fk.hex())
        assert int(got.min()) >= -(1 << sigma) and int(got.max()) < (1 << sigma)
        assert np.array_equal(flood_wide(fk, sigma, 256), got[:256]), "a shorter N is a prefix"
    wide = flood_wide(fkey(1), sigma, 4096)
    assert len(set(int(v) for v in wide)) > (1 if sigma > 1 else 0)
    if sigma >= 21:   # both halves of the range are reached
        assert int(wide.min()) < -(1 << (sigma - 1)) and int(wide.max()) >= (1 << (sigma - 1))


def test_flood_tag_and_argument_checks():
    assert len({tm.FLOOD_TAG, tm.SEED_TAG, tm.SAMPLE_TAG}) == 3
    assert tm.FLOOD_TAG >> 48 not in (tm.SEED_TAG >> 48, tm.SAMPLE_TAG >> 48)
    # the same key under the sampled tag gives other words: no block is shared
    small = _eva._seal._sampled_small(fkey(2), 1, N)
    assert not np.array_equal(flood_wide(fkey(2), 5, N) & 1, small & 1)
    for bad in (0, 63):
        with pytest.raises(ValueError, match="smudge_bits must be 1..62"):
            flood_wide(fkey(0), bad, N)
    with pytest.raises(ValueError, match="32 bytes"):
        flood_wide(b"short", 5, N)


# ---- collective keys
class _Parties:
    """three key pairs over one chain with a common seed, and their collective public context; never written"""

    def __init__(self, chain, rotations=(1, 3)):
        self.params = CKKSParameters(CHAINS[chain], set(rotations), N)
        self.pairs = [generate_keys(self.params, seed=100 + p, common_seed=COMMON) for p in range(3)]
        self.pubs = [p for p, _ in self.pairs]
        self.secs = [s for _, s in self.pairs]
        self.primes = [int(q) for q in self.pubs[0].primes]
        self.k = len(self.primes)
        self.o = po.Oracle(N, self.primes)
        self.chains = [Chain(N, self.primes, s._secret_key_ntt()) for s in self.secs]


@pytest.fixture(scope="module", params=sorted(CHAINS))
def parties(request):
    return _Parties(request.param)


def _centred_max(o, i, row_ntt):
    q = o.primes[i]
    coeff = o.intt(i, np.ascontiguousarray(row_ntt, dtype=np.uint64))
    return max(abs(centered(int(v), q)) for v in coeff)


def test_common_seed_key_pairs(parties):
    ps = parties
    pk = [p.public_key() for p in ps.pubs]
    seeds = [p.key_seeds() for p in ps.pubs]
    for p in (1, 2):
        assert np.array_equal(pk[p][1], pk[0][1]), "the same a"
        assert not np.array_equal(pk[p][0], pk[0][0])
        assert sorted(seeds[p]) == sorted(seeds[0])
        for kid in seeds[0]:
            assert np.array_equal(seeds[p][kid], seeds[0][kid]), kid
        assert not np.array_equal(ps.secs[p]._secret_key_ntt(), ps.secs[0]._secret_key_ntt())
    assert all(p.keys_compressed for p in ps.pubs)
    # each pair alone is a valid key pair: pk0 + pk1 s_p is one small error
    for p in range(3):
        s = ps.secs[p]._secret_key_ntt()
        for i in range(ps.k):
            q = ps.primes[i]
            row = (pk[p][0][i].astype(object) + pk[p][1][i].astype(object) * s[i].astype(object)) % q
            assert _centred_max(ps.o, i, np.array(row, dtype=np.uint64)) <= 21


def test_common_seed_none_is_todays_path_and_bad_lengths_are_refused(parties):
    a, sa = generate_keys(parties.params, seed=5)
    b, sb = generate_keys(parties.params, seed=5, common_seed=None)
    assert np.array_equal(a.public_key(), b.public_key()) and np.array_equal(sa._secret_key_ntt(), sb._secret_key_ntt())
    assert np.array_equal(a.relin_key(), b.relin_key())
    assert a.keys_compressed == b.keys_compressed
    # the common seed changes the public stream only: the secret is the one of generate_keys(seed, device_sampling=True)
    c, sc = generate_keys(parties.params, seed=5, device_sampling=True)
    d, sd = generate_keys(parties.params, seed=5, common_seed=COMMON)
    assert np.array_equal(sc._secret_key_ntt(), sd._secret_key_ntt())
    assert not np.array_equal(c.public_key()[1], d.public_key()[1])
    for bad in (b"", bytes(31), bytes(33)):
        with pytest.raises(ValueError, match="common_seed is 32 bytes"):
            generate_keys(parties.params, seed=5, common_seed=bad)


def test_collective_key_equations(parties):
    ps = parties
    P = 3
    col = combine_public_contexts(ps.pubs)
    assert isinstance(col, SEALPublic) and col.collective and not ps.pubs[0].collective
    sum_ch = tm.sum_chain(ps.chains)
    pk = col.public_key()
    for i in range(ps.k):
        q = ps.primes[i]
        row = (pk[0][i].astype(object) + pk[1][i].astype(object) * sum_ch.s[i]) % q
        got = _centred_max(ps.o, i, np.array(row, dtype=np.uint64))
        assert 0 < got <= 21 * P, (i, got)
    # every Galois digit: c0 + c1 s - [i == J] P_special s(X^elt) within 21 P
    special = ps.primes[-1]
    keys = col.galois_keys()
    assert sorted(keys) == sorted(ps.pubs[0].galois_keys())
    q0 = ps.primes[0]
    s_coeff = np.array([centered(int(v), q0) for v in ps.o.intt(0, np.array(sum_ch.s[0], dtype=np.uint64))], dtype=np.int64)
    assert int(np.abs(s_coeff).max()) <= P
    for elt, key in keys.items():
        s_rot = automorphism(s_coeff, elt, N)
        for J in range(key.shape[0]):
            for i in range(ps.k):
                q = ps.primes[i]
                row = (key[J][0][i].astype(object) + key[J][1][i].astype(object) * sum_ch.s[i]) % q
                if i == J:
                    rot_ntt = ps.o.ntt(i, np.array([int(v) % q for v in s_rot], dtype=np.uint64)).astype(object)
                    row = (row - (special % q) * rot_ntt) % q
                got = _centred_max(ps.o, i, np.array(row, dtype=np.uint64))
                assert got <= 21 * P, (elt, J, i, got)
    with pytest.raises(ValueError, match=r"relinearization key not present \(a collective context has none\)"):
        col.relin_key()
    assert 0 not in col.key_seeds()
    one = combine_public_contexts(ps.pubs[:1])   # P = 1: the party's own keys
    assert np.array_equal(one.public_key(), ps.pubs[0].public_key())


def test_collective_refusals(parties):
    ps = parties
    foreign, _ = generate_keys(ps.params, seed=9, common_seed=bytes(32))
    with pytest.raises(ValueError, match=r"public contexts do not share a common seed \(context 2 differs from context 0\)"):
        combine_public_contexts([ps.pubs[0], ps.pubs[1], foreign])
    bits = list(ps.params.prime_bits)
    bits[1] -= 1
    other, _ = generate_keys(CKKSParameters(bits, set(), N), seed=9, common_seed=COMMON)
    with pytest.raises(ValueError, match="context 1 has other encryption parameters than context 0: prime [01] differs"):
        combine_public_contexts([ps.pubs[0], other])
    bigger, _ = generate_keys(CKKSParameters(list(ps.params.prime_bits), set(), 2 * N), seed=9, common_seed=COMMON)
    with pytest.raises(ValueError, match="poly_modulus_degree differs"):
        combine_public_contexts([ps.pubs[0], bigger])
    with pytest.raises(ValueError, match="1..64 public contexts"):
        combine_public_contexts([])
    # a Galois element one party lacks is not part of the collective context
    fewer, _ = generate_keys(CKKSParameters(list(ps.params.prime_bits), {1}, N), seed=9, common_seed=COMMON)
    col = combine_public_contexts([ps.pubs[0], fewer])
    assert sorted(col.galois_keys()) == sorted(fewer.galois_keys()) and len(col.galois_keys()) < len(ps.pubs[0].galois_keys())
    dropped = set(ps.pubs[0].galois_keys()) - set(fewer.galois_keys())
    assert sorted(col.dropped_galois_elements) == sorted(dropped) and len(dropped) == 1, "the element one party lacks is named"
    assert sorted(combine_public_contexts([fewer, ps.pubs[0]]).dropped_galois_elements) == sorted(dropped), "whichever context lacks it"
    assert combine_public_contexts(ps.pubs).dropped_galois_elements == []


def test_collective_context_save_load(parties, tmp_path):
    col = combine_public_contexts(parties.pubs)
    path = str(tmp_path / "collective.pub")
    save(col, path)
    back = load(path)
    assert isinstance(back, SEALPublic) and back.collective
    assert np.array_equal(back.public_key(), col.public_key())
    a, b = back.galois_keys(), col.galois_keys()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[e], b[e]) for e in a)
    with pytest.raises(ValueError, match="a collective context has no relinearization key"):
        save(col, str(tmp_path / "no.seal"), format="seal")
    own = str(tmp_path / "own.pub")   # an ordinary context still round-trips with its relinearization key
    save(parties.pubs[0], own)
    assert not load(own).collective and np.array_equal(load(own).relin_key(), parties.pubs[0].relin_key())


# ---- the host share and the combination
def _random_ct(rng, primes, l):
    return np.stack([np.stack([rng.integers(0, primes[i], size=N, dtype=np.uint64) for i in range(l)]) for _ in range(2)])


def _encrypt_under(rng, o, ch, values, l, scale):
    """(pt - c1 s, c1) at l limbs under the chain's key, c1 uniform: it decrypts to exactly the encoding of `values`"""
    pt = o.encode(l, values, scale)
    c0, c1 = [], []
    for i in range(l):
        q = ch.primes[i]
        a = rng.integers(0, q, size=N, dtype=np.uint64)
        c0.append(np.array((pt[i].astype(object) - a.astype(object) * ch.s[i]) % q, dtype=np.uint64))
        c1.append(a)
    return np.stack([np.stack(c0), np.stack(c1)])


@pytest.mark.parametrize("l_of", ["1", "2", "k-1"])
def test_share_and_combine_equal_the_model(parties, l_of):
    ps = parties
    l = {"1": 1, "2": 2, "k-1": ps.k - 1}[l_of]
    rng = np.random.default_rng(17 + l)
    sigma, scale = 40, 2.0 ** 30   # 3 2^42 is below the smallest Q_1 (2^60)
    values = rng.uniform(-1, 1, N // 2)
    for P in (1, 2, 3):
        sum_ch = tm.sum_chain(ps.chains[:P])
        ct = _encrypt_under(rng, ps.o, sum_ch, values, l, scale)
        keys = [fkey(100 * l + 10 * P + p) for p in range(P)]
        shares = []
        for p in range(P):
            h = share_host(N, ps.primes, ps.secs[p]._secret_key_ntt(), ct, sigma, keys[p])
            assert h.shape == (l, N) and np.array_equal(h, tm.share(ps.chains[p], ct, sigma, keys[p])), (l, P, p)
            shares.append(h)
        m_coeff, vals = combine_host(N, ps.primes, ct, np.stack(shares), sigma, scale)
        m = tm.combine(ps.chains[0], ct, shares)
        # the sum is (c0 + c1 s + sum_p NTT(E_p)) mod q, word for word
        plain = tm.plain_message(sum_ch, ct)
        floods = [tm.flood(fk, sigma, N) for fk in keys]
        for i in range(l):
            q = ps.primes[i]
            noise = [sum(E[j] for E in floods) % q for j in range(N)]
            want_row = (plain[i].astype(object) + ntt(noise, ps.chains[0].psi[i], q)) % q
            assert np.array_equal(m[i], np.array(want_row, dtype=np.uint64)), (l, P, i)
        assert np.array_equal(m_coeff, tm.coefficients(ps.chains[0], m)), (l, P)
        want_vals = ps.o.decode(m, scale)
        assert np.array_equal(vals.view(np.uint64), want_vals.view(np.uint64)), "the oracle's doubles, bit for bit"
        # against the plain decryption under the P parties' whole key
        exact = ps.o.decode(plain, scale)
        assert float(np.abs(exact - values).max()) < 1e-6
        diff, bound = float(np.abs(vals - exact).max()), tm.slot_bound(N, P, sigma, scale)
        print(f"l={l} P={P} sigma={sigma}: largest slot difference {diff:.3e}, bound {bound:.3e}")
        assert 0 < diff <= bound


def test_room_refusals_fire_at_their_thresholds(parties):
    ps = parties
    rng = np.random.default_rng(3)
    ct = _random_ct(rng, ps.primes, 1)
    q0 = ps.primes[0]
    s0 = ps.secs[0]._secret_key_ntt()
    top = q0.bit_length() - 3   # the largest sigma with 2^(sigma + 2) <= q_0 (q_0 is no power of two)
    assert (1 << (top + 2)) <= q0 < (1 << (top + 3))
    h = share_host(N, ps.primes, s0, ct, top, fkey(1))
    with pytest.raises(ValueError, match="smudge_bits leaves no room at this level"):
        share_host(N, ps.primes, s0, ct, top + 1, fkey(1))
    # combine: P 2^(sigma + 2) > Q_l
    for P in (1, 2, 3):
        fits = max(s for s in range(1, 63) if P * (1 << (s + 2)) <= q0)
        hs = np.stack([h] * P)
        combine_host(N, ps.primes, ct, hs, fits, 2.0 ** 20)
        if fits < 62:
            with pytest.raises(ValueError, match="smudge_bits leaves no room at this level for this many parties"):
                combine_host(N, ps.primes, ct, hs, fits + 1, 2.0 ** 20)
    # two limbs leave room for sigma = 62
    ct2 = _random_ct(rng, ps.primes, 2)
    share_host(N, ps.primes, s0, ct2, 62, fkey(2))


def test_size_3_and_shape_refusals(parties):
    ps = parties
    rng = np.random.default_rng(4)
    s0 = ps.secs[0]._secret_key_ntt()
    ct3 = np.stack([rng.integers(0, ps.primes[0], size=(2, N), dtype=np.uint64) % np.uint64(ps.primes[1]) for _ in range(3)])
    with pytest.raises(ValueError, match=r"decryption share expects a size-2 ciphertext \(relinearize first\)"):
        share_host(N, ps.primes, s0, ct3, 10, fkey(0))
    ct = _random_ct(rng, ps.primes, 2)
    with pytest.raises(ValueError, match=r"decryption share expects a size-2 ciphertext"):
        combine_host(N, ps.primes, ct3, np.zeros((1, 2, N), dtype=np.uint64), 10, 2.0 ** 20)
    with pytest.raises(ValueError, match="shares are"):
        combine_host(N, ps.primes, ct, np.zeros((1, 1, N), dtype=np.uint64), 10, 2.0 ** 20)
    with pytest.raises(ValueError, match="secret key not present"):
        share_host(N, ps.primes, np.zeros((0,), dtype=np.uint64), ct, 10, fkey(0))
    with pytest.raises(ValueError, match="invalid limb count"):
        share_host(N, ps.primes, s0, _random_ct(rng, ps.primes, ps.k), 10, fkey(0))


# ---- the public interface on the host path
def _linear_program():
    from eva import EvaProgram, Input, Output
    from eva.ckks import CKKSCompiler
    prog = EvaProgram("linear", vec_size=N // 2)
    with prog:
        x = Input("x")
        Output("y", (x << 1) * 0.5 + x)
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    return CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)


@pytest.fixture(scope="module")
def flow():
    compiled, params, sig = _linear_program()
    params.poly_modulus_degree = N
    pairs = [generate_keys(params, seed=40 + p, common_seed=COMMON) for p in range(3)]
    col = combine_public_contexts([p for p, _ in pairs])
    x = np.random.default_rng(1).uniform(-1, 1, N // 2)
    return compiled, params, sig, pairs, col, x


def test_shares_through_the_public_interface(flow, tmp_path):
    from eva_amd._eva._seal import DecryptionShares
    compiled, params, sig, pairs, col, x = flow
    enc = col.encrypt({"x": x.tolist()}, sig)
    sigma = 30
    shares = [sec.decrypt_share(enc, sigma, seed=7 + p) for p, (_, sec) in enumerate(pairs)]
    assert all(isinstance(s, DecryptionShares) and s.smudge_bits == sigma and not s.batch and s.names() == ["x"] for s in shares)
    l = shares[0].words("x")[0].shape[1]
    scale = 2.0 ** sig.inputs["x"].scale
    # the input itself, jointly opened: within the flood's bound plus the encryption's own noise
    got = np.array(col.combine_shares(enc, shares, sig)["x"])
    bound = tm.slot_bound(N, 3, sigma, scale) + 1e-3
    diff = float(np.abs(got - x).max())
    print(f"largest slot difference {diff:.3e}, bound {bound:.3e}")
    assert 0 < diff <= bound
    # any context over the same parameters combines: a party's own public half gives the same doubles
    again = np.array(pairs[1][0].combine_shares(enc, shares, sig)["x"])
    assert np.array_equal(again.view(np.uint64), got.view(np.uint64))
    # one party missing: noise
    assert float(np.abs(np.array(col.combine_shares(enc, shares[:2], sig)["x"]) - x).max()) > 1.0
    # randomness contract: the same seed gives the same share, another seed another; seed 0 is the OS
    sec0 = pairs[0][1]
    assert np.array_equal(sec0.decrypt_share(enc, sigma, seed=7).words("x")[0], shares[0].words("x")[0])
    assert not np.array_equal(sec0.decrypt_share(enc, sigma, seed=8).words("x")[0], shares[0].words("x")[0])
    assert not np.array_equal(sec0.decrypt_share(enc, sigma).words("x")[0], sec0.decrypt_share(enc, sigma).words("x")[0])
    # the share is the host twin's on the first key of the stream SecureRng(seed, 5)
    from sampled_keys import stream_keys
    words = np.asarray(enc.get("x")[4], dtype=np.uint64).reshape(2, l, N)
    want = share_host(N, list(col.primes), sec0._secret_key_ntt(), words, sigma, stream_keys(7, 5, 1)[0])
    assert np.array_equal(shares[0].words("x")[0][0], want)
    # save / load
    path = str(tmp_path / "party0.shares")
    save(shares[0], path)
    back = load(path)
    assert isinstance(back, DecryptionShares) and back.smudge_bits == sigma and back.names() == ["x"] and back.poly_modulus_degree == N
    assert np.array_equal(back.words("x")[0], shares[0].words("x")[0])
    mixed = np.array(col.combine_shares(enc, [back, shares[1], shares[2]], sig)["x"])
    assert np.array_equal(mixed.view(np.uint64), got.view(np.uint64))
    with pytest.raises(ValueError, match="DecryptionShares have no SEAL format"):
        save(shares[0], str(tmp_path / "no.seal"), format="seal")
    raw = bytearray(open(path, "rb").read())
    raw[-8:] = b"\xff" * 8
    bad = tmp_path / "bad.shares"
    bad.write_bytes(bytes(raw))
    with pytest.raises(RuntimeError, match="decryption share holds a word that is not reduced"):
        load(str(bad))
    # refusals
    other = sec0.decrypt_share(enc, sigma + 1, seed=1)
    with pytest.raises(ValueError, match=r"share 1: smudge_bits differs from share 0 \(31 against 30\)"):
        col.combine_shares(enc, [shares[0], other], sig)
    with pytest.raises(ValueError, match="smudge_bits must be 1..62"):
        sec0.decrypt_share(enc, 0)
    with pytest.raises(TypeError):
        sec0.decrypt_share(enc)   # no default: the caller's security parameter


def test_size_3_and_room_refusals_through_the_public_interface(flow):
    from eva.seal import SEALValuation
    compiled, params, sig, pairs, col, x = flow
    sec0 = pairs[0][1]
    size3 = SEALValuation()
    size3._set_params(col)
    size3._set_cipher("x", np.zeros((3, 2, N), dtype=np.uint64), 2.0 ** 30)
    with pytest.raises(ValueError, match=r"decryption share expects a size-2 ciphertext \(relinearize first\)"):
        sec0.decrypt_share(size3, 20)
    low = SEALValuation()
    low._set_params(col)
    low._set_cipher("x", np.zeros((2, 1, N), dtype=np.uint64), 2.0 ** 30)
    top = int(col.primes[0]).bit_length() - 3
    sh = sec0.decrypt_share(low, top, seed=1)
    with pytest.raises(ValueError, match="smudge_bits leaves no room at this level"):
        sec0.decrypt_share(low, top + 1, seed=1)
    with pytest.raises(ValueError, match="smudge_bits leaves no room at this level for this many parties"):
        col.combine_shares(low, [sh, sh], sig)
    col.combine_shares(low, [sh], sig)


def test_a_relinearizing_program_is_refused_by_the_collective_context(flow):
    from eva import EvaProgram, Input, Output
    from eva.ckks import CKKSCompiler
    _, _, _, pairs, col, x = flow
    prog = EvaProgram("square", vec_size=N // 2)
    with prog:
        v = Input("x")
        Output("y", v * v)
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.poly_modulus_degree = N
    ps = [generate_keys(params, seed=60 + p, common_seed=COMMON)[0] for p in range(2)]
    c2 = combine_public_contexts(ps)
    enc = c2.encrypt({"x": x.tolist()}, sig)
    with pytest.raises(ValueError, match=r"relinearization key not present \(a collective context has none\)"):
        c2.execute(compiled, enc)


def _signature(names, scale_bits=30, vec=N // 2):
    from eva.ckks import CKKSEncodingInfo, CKKSSignature
    from eva_amd._eva import Type
    return CKKSSignature(vec, {name: CKKSEncodingInfo(Type.Cipher, scale_bits, 0) for name in names})


def test_each_common_seed_pair_round_trips_alone(parties):
    """its own encrypt -> decrypt, under the public key (pub.encrypt) and under the secret key (sec.encrypt).  Bound per slot, hard,
    at scale 2^30: |e_pk u + e0 + e1 s| <= 21 (2 N + 1) per coefficient plus N + 1 from the division by the special prime, N
    coefficients to a slot (a symmetric encryption's error is 21 alone)"""
    sig = _signature(["x"])
    bound = N * (21 * (2 * N + 1) + N + 1) / 2.0 ** 30
    assert bound < 0.05
    x = np.random.default_rng(5).uniform(-1, 1, N // 2)
    for p, (pub, sec) in enumerate(parties.pairs):
        for enc in (pub.encrypt({"x": x.tolist()}, sig), sec.encrypt({"x": x.tolist()}, sig, seed=1 + p)):
            got = np.array(sec.decrypt(enc, sig)["x"])
            assert float(np.abs(got - x).max()) <= bound, p
        # and only its own: another party's secret opens nothing
        other = parties.secs[(p + 1) % 3]
        assert float(np.abs(np.array(other.decrypt(pub.encrypt({"x": x.tolist()}, sig), sig)["x"]) - x).max()) > 1.0


def test_no_two_values_share_a_flooding_key(flow):
    """names sorted, 4 words per value of the one stream SecureRng(seed, 5): value i of a valuation takes key i"""
    from sampled_keys import stream_keys
    compiled, params, _, pairs, col, x = flow
    sig = _signature(["b", "a", "c"])
    enc = col.encrypt({"b": x.tolist(), "a": (0.5 * x).tolist(), "c": x.tolist()}, sig)
    sec0 = pairs[0][1]
    sigma, seed = 30, 21
    sh = sec0.decrypt_share(enc, sigma, seed=seed)
    assert sh.names() == ["a", "b", "c"]
    keys = stream_keys(seed, 5, 3)
    assert len(set(keys)) == 3
    s_ntt, primes = sec0._secret_key_ntt(), list(col.primes)
    words = {}
    for i, name in enumerate(["a", "b", "c"]):
        kind, size, limbs, scale, w = enc.get(name)
        ct = np.asarray(w, dtype=np.uint64).reshape(2, limbs, N)
        words[name] = sh.words(name)[0][0]
        assert np.array_equal(words[name], share_host(N, primes, s_ntt, ct, sigma, keys[i])), f"value {name} takes key {i}"
        for j in range(3):
            if j != i:
                assert not np.array_equal(words[name], share_host(N, primes, s_ntt, ct, sigma, keys[j]))
    # "b" and "c" encrypt the same values; their shares still carry different noise: h_b - c1_b s differs from h_c - c1_c s
    noise = {}
    for name in ("b", "c"):
        ct = np.asarray(enc.get(name)[4], dtype=np.uint64).reshape(2, -1, N)
        q = primes[0]
        noise[name] = (words[name][0].astype(object) - ct[1][0].astype(object) * s_ntt[0].astype(object)) % q
    assert not np.array_equal(noise["b"], noise["c"])
    # a value that is not encrypted draws nothing: the keys of the others do not move
    from eva.seal import SEALValuation
    mixed = SEALValuation()
    mixed._set_params(col)
    for name in ("a", "c"):
        kind, size, limbs, scale, w = enc.get(name)
        mixed._set_cipher(name, np.asarray(w, dtype=np.uint64).reshape(2, limbs, N), scale)
    mixed._set_raw("b", [1.0, 2.0])
    sh2 = sec0.decrypt_share(mixed, sigma, seed=seed)
    assert sh2.names() == ["a", "c"]
    assert np.array_equal(sh2.words("a")[0][0], words["a"])
    ct_c = np.asarray(enc.get("c")[4], dtype=np.uint64).reshape(2, -1, N)
    assert np.array_equal(sh2.words("c")[0][0], share_host(N, primes, s_ntt, ct_c, sigma, keys[1])), "the second encrypted value takes key 1"


def test_combine_refuses_foreign_shares_by_index(flow):
    compiled, params, sig, pairs, col, x = flow
    enc = col.encrypt({"x": x.tolist()}, sig)
    shares = [sec.decrypt_share(enc, 30, seed=1 + p) for p, (_, sec) in enumerate(pairs)]
    # other primes / another degree: a share made under them, named by its index
    bits = list(params.prime_bits)
    other_params = CKKSParameters(bits[:-1] + [bits[-1] - 1], set(), N)
    (pub_o, sec_o) = generate_keys(other_params, seed=3, common_seed=COMMON)
    sig_o = _signature(["x"], sig.inputs["x"].scale, N // 2)
    foreign = sec_o.decrypt_share(pub_o.encrypt({"x": x.tolist()}, sig_o), 30, seed=1)
    with pytest.raises(ValueError, match=r"combine_shares: share 2 was made under other encryption parameters: prime \d+ differs"):
        col.combine_shares(enc, [shares[0], shares[1], foreign], sig)
    big_params = CKKSParameters(bits, set(), 2 * N)
    (pub_b, sec_b) = generate_keys(big_params, seed=3, common_seed=COMMON)
    bigger = sec_b.decrypt_share(pub_b.encrypt({"x": x.tolist() * 2}, _signature(["x"], sig.inputs["x"].scale, N)), 30, seed=1)
    with pytest.raises(ValueError, match=r"share 1 was made under other encryption parameters: poly_modulus_degree differs \(2048 against 1024\)"):
        col.combine_shares(enc, [shares[0], bigger], sig)
    # a share that lacks the value, and one at another level
    sig_y = _signature(["y"], sig.inputs["x"].scale)
    other_name = pairs[1][1].decrypt_share(col.encrypt({"y": x.tolist()}, sig_y), 30, seed=1)
    with pytest.raises(IndexError, match="share 1, value x: the share holds no such value"):
        col.combine_shares(enc, [shares[0], other_name, shares[2]], sig)
    from eva.seal import SEALValuation
    kind, size, limbs, scale, w = enc.get("x")
    low = SEALValuation()
    low._set_params(col)
    low._set_cipher("x", np.ascontiguousarray(np.asarray(w, dtype=np.uint64).reshape(2, limbs, N)[:, :limbs - 1]), scale)
    lower = pairs[1][1].decrypt_share(low, 30, seed=1)
    with pytest.raises(ValueError, match="share 1, value x: limb count differs from the ciphertext's"):
        col.combine_shares(enc, [shares[0], lower, shares[2]], sig)
    with pytest.raises(ValueError, match="shares of 1..64 parties are needed"):
        col.combine_shares(enc, [], sig)
