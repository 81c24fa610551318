"""CPU: the collective relinearization key on the host twins — no GPU.

The derived seeds equal the numpy-ChaCha20 restatement of tests/relin_rounds_model.py, are the same for every party of one
common_seed and differ from the relinearization key's own seeds.  Host round 1 and round 2 equal the model word for word
on both chains of test_threshold_cpu.py at N = 1024 for D in {1, k - 1}, and the public interface is those twins on the
keys of its streams.  The key satisfies c0 + c1 s - w_J s^2 = s e0 + u e1 + e2 + e3 over the integers within
2 N B P^2 + 2 B P (B = 21, the bound of a sampled error) for P in {1, 2, 3, 9}, non-zero.  A relinearization with it (the
oracle's, on a size-3 product) decrypts under s = sum_p s_p to the size-3 decryption within the bound derived in
DESIGN.md 1.15.  Refusals, and save / load of both share kinds and of the collective context with its key."""
import pickle
import struct

import numpy as np
import pytest

import relin_rounds_model as rm
import threshold_model as tm
from eva import load, save
from eva.ckks import CKKSParameters
from eva.seal import SEALPublic, generate_keys
from eva_amd import _eva
from oracle import pyoracle as po
from refresh_model import Chain, decrypt_integers
from sampled_keys import stream_keys

N = 1024
CHAINS = {"mixed": [60, 30, 45, 50, 33, 60], "all60": [60] * 4}
COMMON = bytes(range(7, 39))
seal = _eva._seal
combine_public_contexts, combine_relin_shares = seal.combine_public_contexts, seal.combine_relin_shares
round1_host, round2_host, round_seeds = seal._relin_round1_host, seal._relin_round2_host, seal._relin_round_seeds
RelinShare = seal.RelinShare


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


def keys32(tag, n):
    return np.array([[(tag * 31 + J * 17 + j * 7 + 5) % 256 for j in range(32)] for J in range(n)], dtype=np.uint8)


class _Parties:
    """nine key pairs over one chain with a common seed; never written"""

    def __init__(self, chain):
        self.params = CKKSParameters(CHAINS[chain], {1}, N)
        self.pairs = [generate_keys(self.params, seed=100 + p, common_seed=COMMON) for p in range(9)]
        self.pubs = [p for p, _ in self.pairs]
        self.secs = [s for _, s in self.pairs]
        self.primes = [int(q) for q in self.pubs[0].primes]
        self.k = len(self.primes)
        self.D = self.k - 1
        self.chains = [Chain(N, self.primes, s._secret_key_ntt()) for s in self.secs]
        self.relin_seeds = self.pubs[0].key_seeds()[0]
        self.seeds = round_seeds(self.relin_seeds)
        self._keys = {}

    def run(self, P):
        """both rounds through the public interface for the first P parties -> (round-1 shares, agg1, round-2 shares, col)"""
        if P not in self._keys:
            r1 = [sec.relin_round1(seed=300 + p) for p, sec in enumerate(self.secs[:P])]
            agg = combine_relin_shares([s for _, s in r1])
            r2 = [sec.relin_round2(r1[p][0], agg, seed=400 + p) for p, sec in enumerate(self.secs[:P])]
            col = combine_public_contexts(self.pubs[:P], relin_round1=agg, relin_round2=r2)
            self._keys[P] = ([s for _, s in r1], agg, r2, col)
        return self._keys[P]


@pytest.fixture(scope="module", params=sorted(CHAINS))
def parties(request):
    return _Parties(request.param)


# ---- the derived seeds
def test_derived_seeds(parties):
    ps = parties
    assert ps.seeds.shape == (ps.D, 32) and ps.seeds.dtype == np.uint8
    assert np.array_equal(ps.seeds, rm.derive_seeds(ps.relin_seeds)), "the model's derivation"
    for pub in ps.pubs[1:]:
        assert np.array_equal(round_seeds(pub.key_seeds()[0]), ps.seeds), "the same for all parties of one common_seed"
    for J in range(ps.D):
        assert not np.array_equal(ps.seeds[J], ps.relin_seeds[J]), "never the a of the party's own relinearization key"
    assert len({bytes(s) for s in ps.seeds} | {bytes(s) for s in ps.relin_seeds}) == 2 * ps.D
    assert rm.ROUND_NONCE != rm.COMMON_NONCE and len(rm.ROUND_NONCE) == 8
    # the rows themselves differ: digit 0's common row is not the relinearization key's c1
    own_c1 = ps.pubs[0].relin_key()[0][1][0]
    assert not np.array_equal(rm.expand_limb(bytes(ps.seeds[0]), 0, ps.primes[0], N), own_c1)
    foreign, _ = generate_keys(ps.params, seed=100, common_seed=bytes(32))
    assert not np.array_equal(round_seeds(foreign.key_seeds()[0]), ps.seeds)


# ---- the host twins against the model
@pytest.mark.parametrize("D_of", ["1", "k-1"])
def test_host_rounds_equal_the_model(parties, D_of):
    ps = parties
    D = 1 if D_of == "1" else ps.D
    seeds = ps.seeds[:D]
    r1 = [keys32(10 + p, D) for p in range(2)]
    r2 = [keys32(20 + p, D) for p in range(2)]
    shares = []
    for p in range(2):
        got = round1_host(N, ps.primes, ps.secs[p]._secret_key_ntt(), seeds, r1[p])
        assert got.shape == (D, 2, ps.k, N) and got.dtype == np.uint64
        assert np.array_equal(got, rm.round1(ps.chains[p], seeds, r1[p])), (D, p)
        shares.append(got)
    agg = rm.aggregate(shares, ps.primes)
    for p in range(2):
        got = round2_host(N, ps.primes, ps.secs[p]._secret_key_ntt(), agg, r1[p], r2[p])
        assert got.shape == (D, ps.k, N)
        assert np.array_equal(got, rm.round2(ps.chains[p], agg, r1[p], r2[p])), (D, p)
    with pytest.raises(ValueError, match="secret key not present"):
        round1_host(N, ps.primes, np.zeros((0,), dtype=np.uint64), seeds, r1[0])
    with pytest.raises(ValueError, match="invalid key digit count"):
        round1_host(N, ps.primes, ps.secs[0]._secret_key_ntt(), np.zeros((ps.k, 32), dtype=np.uint8), keys32(1, ps.k))


def test_the_public_interface_is_the_host_twins_on_its_streams(parties):
    ps = parties
    shares1, agg, shares2, col = ps.run(3)
    for p in range(3):
        s1 = shares1[p]
        assert isinstance(s1, RelinShare) and s1.round == 1 and s1.N == N and s1.n_digits == ps.D and [int(q) for q in s1.primes] == ps.primes
        k1 = np.frombuffer(b"".join(stream_keys(300 + p, 6, ps.D)), dtype=np.uint8).reshape(ps.D, 32)
        k2 = np.frombuffer(b"".join(stream_keys(400 + p, 7, ps.D)), dtype=np.uint8).reshape(ps.D, 32)
        s_ntt = ps.secs[p]._secret_key_ntt()
        assert np.array_equal(s1.words(), round1_host(N, ps.primes, s_ntt, ps.seeds, k1)), p
        assert shares2[p].round == 2 and shares2[p].words().shape == (ps.D, ps.k, N)
        assert np.array_equal(shares2[p].words(), round2_host(N, ps.primes, s_ntt, agg.words(), k1, k2)), p
    assert agg.round == 1 and np.array_equal(agg.words(), rm.aggregate([s.words() for s in shares1], ps.primes))
    assert isinstance(col, SEALPublic) and col.collective and col.has_relin_key and ps.pubs[0].has_relin_key
    assert np.array_equal(col.relin_key(), rm.key(agg.words(), [s.words() for s in shares2], ps.primes))
    # what the context says of its keys: the Galois keys are compressed, the relinearization key is whole and has no seeds
    assert col.keys_compressed and 0 not in col.key_seeds() and sorted(col.key_seeds()) == sorted(col.galois_keys())
    # without the keywords: today's context, no key
    bare = combine_public_contexts(ps.pubs[:3])
    assert bare.collective and not bare.has_relin_key
    assert np.array_equal(bare.public_key(), col.public_key())
    with pytest.raises(ValueError, match=r"relinearization key not present \(a collective context has none\)"):
        bare.relin_key()
    # seed 0 is the OS: two calls differ; the same test seed repeats
    sec0 = ps.secs[0]
    assert not np.array_equal(sec0.relin_round1()[1].words(), sec0.relin_round1()[1].words())
    assert np.array_equal(sec0.relin_round1(seed=300)[1].words(), shares1[0].words())


# ---- the key equation over the integers
@pytest.mark.parametrize("P", [1, 2, 3, 9])
def test_key_equation_in_integers(parties, P):
    ps = parties
    _, _, _, col = ps.run(P)
    key = col.relin_key()
    assert key.shape == (ps.D, 2, ps.k, N)
    sum_ch = tm.sum_chain(ps.chains[:P])
    bound = rm.key_noise_bound(N, P)
    assert bound == 2 * N * 21 * P * P + 2 * 21 * P
    for J in range(ps.D):
        worst = max(abs(v) for v in rm.key_noise_integers(sum_ch, key, J))
        print(f"P={P} digit {J}: largest |c0 + c1 s - w s^2| {worst}, bound {bound}")
        assert 0 < worst <= bound, (P, J, worst)


# ---- a relinearization with the collective key
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


@pytest.mark.parametrize("l_of", ["2", "k-1"])
def test_relinearization_with_the_collective_key(parties, l_of):
    ps = parties
    P = 3
    l = 2 if l_of == "2" else ps.k - 1
    _, _, _, col = ps.run(P)
    o = po.Oracle(N, ps.primes)
    sum_ch = tm.sum_chain(ps.chains[:P])
    rng = np.random.default_rng(5 + l)
    x, y = rng.uniform(-1, 1, N // 2), rng.uniform(-1, 1, N // 2)
    scale = 2.0 ** 25
    ct3 = o.multiply(_encrypt_under(rng, o, sum_ch, x, l, scale), _encrypt_under(rng, o, sum_ch, y, l, scale))
    assert ct3.shape == (3, l, N)
    ct2 = o.relinearize(ct3, np.ascontiguousarray(col.relin_key()))
    want, got = decrypt_integers(sum_ch, ct3), decrypt_integers(sum_ch, ct2)
    diff = max(abs(a - b) for a, b in zip(want, got))
    bound = rm.relin_noise_bound(N, ps.primes, l, P)
    print(f"l={l}: largest coefficient difference {diff}, bound {bound}")
    assert 0 < diff <= bound
    assert bound < tm.Q_of(ps.primes, l) // 4, "the bound means something at this level"
    # and the product is the product: the slots of x * y at scale^2
    vals = o.decode(o.decrypt(ct2, np.stack([np.array(r, dtype=np.uint64) for r in sum_ch.s])), scale * scale)
    assert float(np.abs(vals - x * y).max()) < 1e-3


# ---- refusals
def test_refusals(parties):
    ps = parties
    shares1, agg, shares2, col = ps.run(3)
    pubs = ps.pubs[:3]
    with pytest.raises(ValueError, match="relin_round1 and relin_round2 go together: give both or neither"):
        combine_public_contexts(pubs, relin_round1=agg)
    with pytest.raises(ValueError, match="relin_round1 and relin_round2 go together: give both or neither"):
        combine_public_contexts(pubs, relin_round2=shares2)
    with pytest.raises(ValueError, match="2 round-2 shares for 3 public contexts"):
        combine_public_contexts(pubs, relin_round1=agg, relin_round2=shares2[:2])
    with pytest.raises(ValueError, match="relin_round1 is a round-2 share"):
        combine_public_contexts(pubs, relin_round1=shares2[0], relin_round2=shares2)
    with pytest.raises(ValueError, match="round-2 share 1 is a round-1 share"):
        combine_public_contexts(pubs, relin_round1=agg, relin_round2=[shares2[0], shares1[1], shares2[2]])
    with pytest.raises(ValueError, match=r"combine_relin_shares: share 1 is a round-2 share"):
        combine_relin_shares([shares1[0], shares2[1]])
    with pytest.raises(ValueError, match="1..64 parties"):
        combine_relin_shares([])
    # mismatched parameters, by index
    bits = list(ps.params.prime_bits)
    bits[1] -= 1
    _, sec_o = generate_keys(CKKSParameters(bits, set(), N), seed=9, common_seed=COMMON)
    other1 = sec_o.relin_round1(seed=1)[1]
    with pytest.raises(ValueError, match=r"combine_relin_shares: share 2 was made under other encryption parameters than share 0: prime [01] differs"):
        combine_relin_shares([shares1[0], shares1[1], other1])
    _, sec_b = generate_keys(CKKSParameters(list(ps.params.prime_bits), set(), 2 * N), seed=9, common_seed=COMMON)
    eph_b, big1 = sec_b.relin_round1(seed=1)
    with pytest.raises(ValueError, match=r"share 1 was made under other encryption parameters than share 0: poly_modulus_degree differs \(2048 against 1024\)"):
        combine_relin_shares([shares1[0], big1])
    with pytest.raises(ValueError, match="relin_round2: the aggregate was made under other encryption parameters: poly_modulus_degree differs"):
        ps.secs[0].relin_round2(ps.secs[0].relin_round1(seed=1)[0], big1)
    big2 = sec_b.relin_round2(eph_b, big1, seed=2)
    with pytest.raises(ValueError, match="round-2 share 2 was made under other encryption parameters than context 0: poly_modulus_degree differs"):
        combine_public_contexts(pubs, relin_round1=agg, relin_round2=[shares2[0], shares2[1], big2])
    fewer = RelinShare._from_words(1, ps.primes, shares1[1].words()[:1])
    if ps.D > 1:
        with pytest.raises(ValueError, match="share 1 has another digit count than share 0"):
            combine_relin_shares([shares1[0], fewer])
    # the ephemeral state: used once, by the context that made it, never pickled
    eph, mine = ps.secs[0].relin_round1(seed=300)
    with pytest.raises(ValueError, match="relin_round2: the ephemeral state was made by another secret context"):
        ps.secs[1].relin_round2(eph, agg)
    assert not eph.used
    again = ps.secs[0].relin_round2(eph, agg, seed=400)
    assert eph.used and np.array_equal(again.words(), shares2[0].words())
    with pytest.raises(ValueError, match=r"relin_round2: the ephemeral state was already used \(a second share would reuse u\)"):
        ps.secs[0].relin_round2(eph, agg, seed=401)
    with pytest.raises(TypeError, match="cannot be pickled"):
        pickle.dumps(eph)
    with pytest.raises(TypeError):
        save(eph, "nowhere")
    with pytest.raises(ValueError, match="the aggregate is not made of round-1 shares"):
        ps.secs[0].relin_round2(ps.secs[0].relin_round1(seed=1)[0], shares2[0])
    # a context whose keys did not come from a common seed
    _, lone = generate_keys(ps.params, seed=5)
    with pytest.raises(ValueError, match="relin_round1: this context's keys were not generated with a common seed"):
        lone.relin_round1()
    _, sampled = generate_keys(ps.params, seed=5, device_sampling=True)
    with pytest.raises(ValueError, match="not generated with a common seed"):
        sampled.relin_round1()
    # out-of-range words
    bad = shares2[1].words().copy()
    bad[-1, -1, -1] = ps.primes[-1]
    with pytest.raises(ValueError, match="round-2 share 1 holds a word that is not reduced modulo its prime"):
        combine_public_contexts(pubs, relin_round1=agg, relin_round2=[shares2[0], RelinShare._from_words(2, ps.primes, bad), shares2[2]])
    bad1 = agg.words().copy()
    bad1[0, 1, 0, 0] = ps.primes[0]
    bad_agg = RelinShare._from_words(1, ps.primes, bad1)
    with pytest.raises(ValueError, match="relin_round1 holds a word that is not reduced modulo its prime"):
        combine_public_contexts(pubs, relin_round1=bad_agg, relin_round2=shares2)
    with pytest.raises(ValueError, match="relin_round2: the aggregate holds a word that is not reduced modulo its prime"):
        ps.secs[0].relin_round2(ps.secs[0].relin_round1(seed=1)[0], bad_agg)


# ---- save / load
def test_shares_save_and_load(parties, tmp_path):
    ps = parties
    shares1, agg, shares2, _ = ps.run(3)
    for name, share in (("one", shares1[0]), ("agg", agg), ("two", shares2[2])):
        path = str(tmp_path / (name + ".share"))
        save(share, path)
        back = load(path)
        assert isinstance(back, RelinShare) and (back.round, back.N, back.n_digits) == (share.round, N, ps.D)
        assert [int(q) for q in back.primes] == ps.primes and np.array_equal(back.words(), share.words())
    # loaded shares serve: the same context from files
    col = combine_public_contexts(ps.pubs[:3], relin_round1=load(str(tmp_path / "agg.share")),
                                  relin_round2=[shares2[0], shares2[1], load(str(tmp_path / "two.share"))])
    assert np.array_equal(col.relin_key(), ps.run(3)[3].relin_key())
    with pytest.raises(ValueError, match="a RelinShare has no SEAL format"):
        save(agg, str(tmp_path / "no.seal"), format="seal")
    raw = bytearray(open(str(tmp_path / "two.share"), "rb").read())
    raw[-8:] = b"\xff" * 8
    (tmp_path / "bad.share").write_bytes(bytes(raw))
    with pytest.raises(RuntimeError, match="relinearization share holds a word that is not reduced"):
        load(str(tmp_path / "bad.share"))


def test_collective_context_with_the_key_saves_and_loads_whole(parties, tmp_path):
    ps = parties
    _, agg, shares2, col = ps.run(3)
    path = str(tmp_path / "collective.pub")
    save(col, path)
    back = load(path)
    assert isinstance(back, SEALPublic) and back.collective and back.has_relin_key
    assert np.array_equal(back.relin_key(), col.relin_key()) and np.array_equal(back.public_key(), col.public_key())
    a, b = back.galois_keys(), col.galois_keys()
    assert sorted(a) == sorted(b) and all(np.array_equal(a[e], b[e]) for e in a)
    assert back.dropped_galois_elements == [] and back.keys_compressed and 0 not in back.key_seeds()
    # the dropped elements survive with the key
    fewer, sec_f = generate_keys(CKKSParameters(list(ps.params.prime_bits), set(), N), seed=100, common_seed=COMMON)
    lacking = combine_public_contexts([fewer, ps.pubs[1], ps.pubs[2]], relin_round1=agg, relin_round2=shares2)
    assert len(lacking.dropped_galois_elements) == 1
    save(lacking, path)
    again = load(path)
    assert again.collective and again.dropped_galois_elements == lacking.dropped_galois_elements
    assert np.array_equal(again.relin_key(), lacking.relin_key())
    # the SEAL format keeps refusing a collective context, with or without the key
    with pytest.raises(ValueError, match="the SEAL format cannot mark a context as collective"):
        save(col, str(tmp_path / "no.seal"), format="seal")
    # a file from before: no key, the absent-key marker in its place — written and read as it always was
    bare = combine_public_contexts(ps.pubs[:3])
    old = str(tmp_path / "old.pub")
    save(bare, old)
    raw = open(old, "rb").read()
    at = 12 + 4 + 8 + 8 * ps.k + 8 + 8 * 2 * ps.k * N   # magic, version, kind; N; the primes; the public key
    assert struct.unpack_from("<I", raw, at)[0] == 0x40000000
    got = load(old)
    assert got.collective and not got.has_relin_key and np.array_equal(got.public_key(), bare.public_key())
    with pytest.raises(ValueError, match="a collective context has no relinearization key"):
        save(bare, str(tmp_path / "no2.seal"), format="seal")
    # an ordinary context is written as before as well
    own = str(tmp_path / "own.pub")
    save(ps.pubs[0], own)
    assert not load(own).collective and load(own).has_relin_key and np.array_equal(load(own).relin_key(), ps.pubs[0].relin_key())
