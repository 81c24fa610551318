"""GPU: the whole key set generated on the MI355X from 32-byte randomness keys.  evah_keygen_set draws the
error of every digit of every key on the device (k_sample_small), transforms them in two launches and forms all keys in
one (k_keygen_set); evah_keygen_public makes the public key with the same kernel; evah_key_download_c0 fetches c0 of a
key generated in place when somebody needs it.  The set is compared word for word with evah_keygen_switch fed the host
expansion of the same keys, as installed with a seeded upload, across chunk boundaries, with the host twin through
generate_keys(..., device_keygen=True, device_sampling=True), and used by the key-switching entry points and execute()
against the oracle in every mode; the transfer counters show that no c0 leaves the device before the first save."""
import numpy as np
import pytest

from eva import save
from eva.seal import generate_keys
from eva_amd import backend
from evatest import oracle_execute
from oracle import pyoracle as po
from sampled_keys import SHAPES, elt_of_step, keys_of, params_of, sampled_small
from test_gpu_seeded_keys import _ctx, _numpy_words, _split, _upload, _work, _valuation, _same

pytestmark = pytest.mark.gpu

RELIN, GALOIS = backend.KEY_RELIN, backend.KEY_GALOIS
SEED = 7


def _secret(o, rng):
    """a ternary secret: coefficients, and [k][N] NTT form under every chain prime"""
    s = rng.integers(-1, 2, size=o.N)
    return s, np.stack([o.ntt(i, np.array([int(v) % q for v in s], dtype=np.uint64)) for i, q in enumerate(o.primes)])


def _secret_ctx(N, primes, rng, **knobs):
    o = po.Oracle(N, primes)
    s, s_ntt = _secret(o, rng)
    g = _ctx(N, primes, **knobs)
    g.upload_secret_key(s_ntt)
    return g, s, s_ntt


def _key_list(N, steps):
    return [(RELIN, 0)] + [(GALOIS, elt_of_step(N, st)) for st in steps]


def _draws(rng, n, D):
    return rng.integers(0, 256, size=(n, D, 32), dtype=np.uint8), rng.integers(0, 256, size=(n, D, 32), dtype=np.uint8)


def _host_errors(ekeys, N):
    """errors[J] = sampled_small(ekeys[J], 1): what evah_keygen_switch takes for the same key"""
    return np.stack([sampled_small(ek.tobytes(), 1, N) for ek in ekeys])


# ---- 1. the set against the existing path

@pytest.mark.parametrize("mac3", [1, 0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_keygen_set_equals_keygen_switch_with_host_expanded_errors(name, mac3):
    N, bits, steps = SHAPES[name]
    primes = po.coeff_modulus_create(N, bits)
    k, D = len(primes), len(primes) - 1
    rng = np.random.default_rng(N + k)
    knobs = {} if mac3 else {"EVAH_MAC3": 0}
    g, _, s_ntt = _secret_ctx(N, primes, rng, **knobs)
    h, f = _ctx(N, primes, **knobs), _ctx(N, primes, **knobs)
    h.upload_secret_key(s_ntt)
    keys = _key_list(N, steps)
    ekeys, seeds = _draws(rng, len(keys), D)
    before = g.transfer_stats()
    c0 = g.keygen_set(keys, ekeys, seeds)
    after = g.transfer_stats()
    assert after[4] - before[4] == 64 * len(keys) * D and after[5] - before[5] == c0.nbytes
    assert g.key_upload_stats() == (0, 0), "a key generated in place is no upload"
    assert c0.shape == (len(keys), D, k, N)
    for j, (kind, elt) in enumerate(keys):
        want = h.keygen_switch(kind, elt, _host_errors(ekeys[j], N), seeds[j], install=False)
        assert np.array_equal(c0[j], want), f"key {j} ({kind}, {elt}): c0"
        _upload(f, elt, c0[j], seeds[j])
        got = g.key_words(kind, elt, 0, D)
        assert np.array_equal(got, _numpy_words(c0[j], seeds[j], primes, N)), f"key {j}: installed words"
        assert np.array_equal(got, f.key_words(kind, elt, 0, D)), f"key {j}: against the seeded upload"
        if mac3:
            sp = g.key_words(kind, elt, 1, D)
            assert np.array_equal(sp, _split(got)) and np.array_equal(sp, f.key_words(kind, elt, 1, D)), f"key {j}: split copy"
        else:
            with pytest.raises(backend.EvaHipError, match="no split copy"):
                g.key_words(kind, elt, 1, D)
        assert np.array_equal(g.key_download_c0(kind, elt, D), c0[j]), f"key {j}: evah_key_download_c0"
    assert g.key_bytes_detail() == f.key_bytes_detail()
    assert h.key_bytes() == 0
    # install = 0 leaves nothing behind and returns the same words; a second set replaces the first in place
    assert np.array_equal(h.keygen_set(keys, ekeys, seeds, install=False), c0) and h.key_bytes() == 0
    assert g.keygen_set(keys, ekeys, seeds, download=False) is None
    assert g.key_bytes_detail() == f.key_bytes_detail()
    for x in (g, h, f):
        x.close()


# ---- 2. chunks of whole keys

@pytest.mark.parametrize("n_keys", [4, 3])
def test_chunked_set_equals_the_one_chunk_set(n_keys):
    """EVAH_KEYGEN_SET_WORDS = two keys' worth of NTT-form errors: 4 keys run as 2 + 2, 3 keys as 2 + 1"""
    N, bits, steps = SHAPES["N1024_mixed"]
    primes = po.coeff_modulus_create(N, bits)
    k, D = len(primes), len(primes) - 1
    rng = np.random.default_rng(n_keys)
    o = po.Oracle(N, primes)
    _, s_ntt = _secret(o, rng)
    keys = _key_list(N, steps)[:n_keys]
    assert len(keys) == n_keys
    ekeys, seeds = _draws(rng, n_keys, D)
    out = []
    for words in (None, 2 * D * k * N, 1):   # one chunk (the default), chunks of two keys, at least one key per chunk
        g = _ctx(N, primes, **({} if words is None else {"EVAH_KEYGEN_SET_WORDS": words}))
        g.upload_secret_key(s_ntt)
        c0 = g.keygen_set(keys, ekeys, seeds)
        out.append((c0, [g.key_words(kd, e, 0, D) for kd, e in keys], [g.key_words(kd, e, 1, D) for kd, e in keys]))
        g.close()
    for other in out[1:]:
        assert np.array_equal(other[0], out[0][0])
        for which in (1, 2):
            for a, b in zip(other[which], out[0][which]):
                assert np.array_equal(a, b)


# ---- 3. the public key

def test_public_key_equation_and_use():
    N, bits, _ = SHAPES["N1024_mixed"]
    primes = po.coeff_modulus_create(N, bits)
    k, l = len(primes), len(primes) - 1
    rng = np.random.default_rng(21)
    g, s, s_ntt = _secret_ctx(N, primes, rng)
    o = po.Oracle(N, primes)
    ekey, seed = bytes(rng.integers(0, 256, size=32, dtype=np.uint8)), bytes(rng.integers(0, 256, size=32, dtype=np.uint8))
    before = g.transfer_stats()
    pk = g.keygen_public(ekey, seed)
    after = g.transfer_stats()
    assert after[4] - before[4] == 64 and after[5] - before[5] == 2 * k * N * 8
    e = sampled_small(ekey, 1, N)
    from test_seeded_cpu import expand_limb
    for i, q in enumerate(primes):
        assert np.array_equal(pk[1, i], expand_limb(seed, i, q, N)), f"a, prime {i}"
        m = [(int(b) + int(a) * int(sv)) % q for b, a, sv in zip(pk[0, i], pk[1, i], s_ntt[i])]
        want = np.array([(-int(v)) % q for v in e], dtype=np.uint64)
        assert np.array_equal(o.intt(i, np.array(m, dtype=np.uint64)), want), f"key equation, prime {i}"
    assert np.array_equal(g.keygen_public(ekey, seed, install=False), pk)
    # installed, it encrypts like the same key uploaded
    f = backend.Context(N, primes)
    f.upload_public_key(pk)
    small = np.stack([sampled_small(bytes(range(32)), p, N) for p in range(3)])
    pt = np.stack([rng.integers(0, primes[i], size=N, dtype=np.uint64) for i in range(l)])
    got = g.encrypt(g.upload_pt(pt, 2.0 ** 30), small).download()
    assert np.array_equal(got, f.encrypt(f.upload_pt(pt, 2.0 ** 30), small).download())
    g.close()
    f.close()


# ---- 4. generate_keys: the device path against the host twin

def _twin(name):
    return generate_keys(params_of(name), SEED, device_sampling=True)


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_key_set_equals_the_host_twin(name, tmp_path):
    N, bits, steps = SHAPES[name]
    pubd, secd = generate_keys(params_of(name), SEED, device_keygen=True, device_sampling=True)
    pubh, sech = _twin(name)
    assert pubd.keys_compressed and pubh.keys_compressed
    assert pubd.key_host_bytes() == 0 and pubh.key_host_bytes() > 0
    assert np.array_equal(secd._secret_key_ntt(), sech._secret_key_ntt())
    assert np.array_equal(pubd.public_key(), pubh.public_key())
    rd, rh = secd._key_randomness(), sech._key_randomness()
    assert sorted(map(str, rd)) == sorted(map(str, rh)) and all(np.array_equal(np.asarray(rd[e]), np.asarray(rh[e])) for e in rh)
    sd, sh = pubd.key_seeds(), pubh.key_seeds()
    assert sorted(sd) == sorted(sh) and len(sd) == 1 + len(steps)
    for e in sh:
        assert np.array_equal(sd[e], sh[e]), f"seeds of key {e}"
    kd, kh = keys_of(pubd), keys_of(pubh)
    for e in kh:
        assert np.array_equal(kd[e][:, 0], kh[e][:, 0]), f"c0 of key {e}"
        assert np.array_equal(kd[e], kh[e]), f"materialised words of key {e}"
    fd, fh = tmp_path / "d.sealpub", tmp_path / "h.sealpub"
    save(pubd, str(fd))
    save(pubh, str(fh))
    assert fd.read_bytes() == fh.read_bytes()


# ---- 5. nothing comes back before it is needed

def test_default_mode_downloads_c0_at_the_first_save_only(tmp_path, tmp_path_factory):
    compiled, params, words, _, _ = _work("readme", tmp_path_factory)
    pub, sec = generate_keys(params, SEED, device_keygen=True, device_sampling=True)
    ref, _ = generate_keys(params, SEED, compress_keys=True)
    N, k = pub.poly_modulus_degree, len(pub.primes)
    D, n_keys = k - 1, len(pub.key_seeds())
    c0_bytes = n_keys * D * k * N * 8
    st = pub.transfer_stats()
    assert pub.key_host_bytes() == 0
    assert st["h2d_bytes"] == 64 * (n_keys * D + 1)   # the secret key's upload counts nothing, as without the option
    assert st["d2h_bytes"] == 2 * k * N * 8           # the public key alone
    assert pub.key_upload_stats() == {"uploads": 0, "bytes": 0}
    assert pub.key_bytes() == [2 * c0_bytes]
    rb = ref.transfer_stats()
    got = pub.execute(compiled, _valuation(words[0]))
    ref.execute(compiled, _valuation(words[0]))
    first, rf = pub.transfer_stats(), ref.transfer_stats()   # before the outputs are read: get() downloads them
    assert pub.key_host_bytes() == 0 and pub.key_upload_stats() == {"uploads": 0, "bytes": 0}
    # what execute() moved is its values, byte for byte what the host-generated pair's execute() counts for them
    assert first["h2d_bytes"] - st["h2d_bytes"] == rf["h2d_bytes"] - rb["h2d_bytes"]
    assert first["d2h_bytes"] - st["d2h_bytes"] == rf["d2h_bytes"] - rb["d2h_bytes"]
    twin, _ = generate_keys(params, SEED, device_sampling=True)
    _same(got, oracle_execute(twin, compiled, _valuation(words[0])))
    before = pub.transfer_stats()["d2h_bytes"]
    save(pub, str(tmp_path / "a.sealpub"))
    mid = pub.transfer_stats()["d2h_bytes"]
    assert mid - before == c0_bytes and pub.key_host_bytes() == c0_bytes
    save(pub, str(tmp_path / "b.sealpub"))
    assert pub.transfer_stats()["d2h_bytes"] == mid and pub.key_host_bytes() == c0_bytes
    assert (tmp_path / "a.sealpub").read_bytes() == (tmp_path / "b.sealpub").read_bytes()
    save(twin, str(tmp_path / "t.sealpub"))
    assert (tmp_path / "a.sealpub").read_bytes() == (tmp_path / "t.sealpub").read_bytes()


# ---- 6. the keys work

def test_set_keys_switch_like_uploaded_ones():
    """relinearize and rotations of both signs on a context whose keys evah_keygen_set made in place, on one that uploaded
    the same words, and by the oracle under those words: the same bits.  (The conjugation key, step 0, is made and
    compared word for word above and against the key equation in tests/test_sampled_keys_cpu.py; no entry point applies
    it: evah_rotate by 0 steps is the identity, as in SEAL.)"""
    N, bits, steps = SHAPES["N1024_mixed"]
    primes = po.coeff_modulus_create(N, bits)
    k, l = len(primes), len(primes) - 1
    o = po.Oracle(N, primes)
    rng = np.random.default_rng(6)
    g, _, _ = _secret_ctx(N, primes, rng)
    f = backend.Context(N, primes)
    keys = _key_list(N, steps)
    ekeys, seeds = _draws(rng, len(keys), l)
    c0 = g.keygen_set(keys, ekeys, seeds)
    words = {}
    for j, (kind, elt) in enumerate(keys):
        words[elt] = _numpy_words(c0[j], seeds[j], primes, N)
        (f.upload_relin_key(words[elt]) if elt == 0 else f.upload_galois_key(elt, words[elt]))

    def rand(size):
        return np.stack([rng.integers(0, primes[i], size=(size, N), dtype=np.uint64) for i in range(l)], axis=1)
    a, a3 = rand(2), rand(3)
    up = lambda c, x: c.upload_ct(x, 2.0 ** 30)
    want = o.relinearize(a3, words[0])
    assert np.array_equal(g.relinearize(up(g, a3)).download(), want) and np.array_equal(f.relinearize(up(f, a3)).download(), want)
    for st in (1, -3):
        want = o.rotate(a, st, words[elt_of_step(N, st)])
        assert np.array_equal(g.rotate(up(g, a), st).download(), want), f"rotate by {st}"
        assert np.array_equal(f.rotate(up(f, a), st).download(), want), f"rotate by {st}, uploaded keys"
    g.close()
    f.close()


_WANT = {}


def _oracle_outputs(name, compiled, params, words):
    """the oracle's outputs under the materialised words of the sampled key set (host twin), once per workload"""
    if name not in _WANT:
        twin, _ = generate_keys(params, SEED, device_sampling=True)
        _WANT[name] = [oracle_execute(twin, compiled, _valuation(w)) for w in words]
    return _WANT[name]


@pytest.mark.parametrize("mode", ["resident", "subdag", "limb", "batch"])
@pytest.mark.parametrize("name", ["readme", "sobel"])
def test_execute_with_the_sampled_key_set_is_bit_exact(name, mode, tmp_path_factory):
    compiled, params, words, _, _ = _work(name, tmp_path_factory)
    want = _oracle_outputs(name, compiled, params, words)
    kw = {"devices": [0, 0], "shard": mode} if mode in ("subdag", "limb") else {}
    pub, _ = generate_keys(params, SEED, device_keygen=True, device_sampling=True, **kw)
    N, k = pub.poly_modulus_degree, len(pub.primes)
    c0_bytes = len(pub.key_seeds()) * (k - 1) * k * N * 8
    # default mode: installed as generated, no c0 on the host; every other mode: c0 came back for the members' uploads
    assert pub.key_host_bytes() == (c0_bytes if kw else 0)
    assert pub.key_bytes() == ([0] if kw else [2 * c0_bytes])
    if mode == "batch":
        vals = [_valuation(w) for w in words]
        for got, oracle in zip(pub.execute_batch(compiled, vals), want):
            _same(got, oracle)
        return
    for call in range(3):   # eager walk, plan capture, replay
        _same(pub.execute(compiled, _valuation(words[0])), want[0])
    if not kw:
        assert pub.key_upload_stats() == {"uploads": 0, "bytes": 0} and pub.key_host_bytes() == 0


# ---- 7. refusals

def test_argument_errors():
    """every refusal with its message; after a refused set no key is left behind"""
    N, bits, _ = SHAPES["N1024_mixed"]
    primes = po.coeff_modulus_create(N, bits)
    k, D = len(primes), len(primes) - 1
    rng = np.random.default_rng(2)
    lib = backend.load()
    C = backend.C
    u8p = C.POINTER(C.c_uint8)
    ekeys, seeds = _draws(rng, 4, D)
    c0 = np.zeros((4, D, k, N), dtype=np.uint64)
    p_e, p_s, p_c0 = ekeys.ctypes.data_as(u8p), seeds.ctypes.data_as(u8p), backend._p(c0)
    elt1, elt3 = elt_of_step(N, 1), elt_of_step(N, 3)

    def ints(v, t=C.c_int):
        return (t * max(len(v), 1))(*v)

    def err(rc):
        assert rc != 0
        return lib.evah_last_error().decode()

    def kset(ctx, kinds, elts, D_=D, e=p_e, s=p_s, install=1, out=p_c0, n=None):
        return err(lib.evah_keygen_set(ctx.h, len(kinds) if n is None else n, ints(kinds), ints(elts, C.c_uint32), D_, e, s, install, out))
    one = ([RELIN], [0])
    bare = backend.Context(N, primes)
    assert kset(bare, *one) == "secret key not present"
    assert err(lib.evah_keygen_public(bare.h, p_e, p_s, 1, p_c0)) == "secret key not present"
    assert err(lib.evah_key_download_c0(bare.h, RELIN, 0, D, p_c0)) == "key not present"
    assert err(lib.evah_key_download_c0(bare.h, GALOIS, elt1, D, p_c0)) == "key not present"
    assert bare.key_bytes() == 0
    bare.close()
    g, _, _ = _secret_ctx(N, primes, rng)
    # evah_keygen_switch's refusals, with its messages
    for elt in (4, 2 * N + 1):
        assert kset(g, [RELIN, GALOIS], [0, elt]) == "Galois element is not valid"
    for d in (0, D + 1):
        assert kset(g, *one, D_=d) == "invalid key digit count"
    assert kset(g, [RELIN, 7], [0, 0]) == "unknown key kind"
    assert "error pointer is null" in kset(g, *one, e=None)
    assert "seed pointer is null" in kset(g, *one, s=None)
    assert "neither installed nor returned" in kset(g, *one, install=0, out=None)
    # its own
    assert "at least one key" in kset(g, [], [])
    assert "key list pointer is null" in err(lib.evah_keygen_set(g.h, 1, None, None, D, p_e, p_s, 1, p_c0))
    many = 65535 // D + 1
    assert "at most 65535 digits" in kset(g, [GALOIS] * many, [2 * i + 1 for i in range(many)])
    assert kset(g, [RELIN, GALOIS, GALOIS, GALOIS], [0, elt1, elt3, elt1]) == "key 3 repeats key 1"
    assert kset(g, [GALOIS, RELIN, RELIN], [elt1, 0, 5]) == "key 2 repeats key 1"
    assert "error pointer is null" in err(lib.evah_keygen_public(g.h, None, p_s, 1, p_c0))
    assert "seed pointer is null" in err(lib.evah_keygen_public(g.h, p_e, None, 1, p_c0))
    assert "neither installed nor returned" in err(lib.evah_keygen_public(g.h, p_e, p_s, 0, None))
    assert "unknown key kind" in err(lib.evah_key_download_c0(g.h, 7, 0, D, p_c0))
    assert "output pointer is null" in err(lib.evah_key_download_c0(g.h, RELIN, 0, D, None))
    # a capturing context (one real call is captured around the refusals, so that the graph is an ordinary one)
    A = g.upload_ct(np.zeros((2, D, N), dtype=np.uint64), 2.0 ** 30)
    g.capture_begin()
    try:
        B = g.negate(A)
        assert "cannot be captured" in kset(g, *one)
        assert "cannot be captured" in err(lib.evah_keygen_public(g.h, p_e, p_s, 1, p_c0))
        assert "cannot be captured" in err(lib.evah_key_download_c0(g.h, RELIN, 0, D, p_c0))
    finally:
        g.graph_free(g.capture_end())
    del A, B
    assert g.key_bytes() == 0
    with pytest.raises(backend.EvaHipError, match="no such key"):
        g.key_words(RELIN, 0, 0)
    # an installed key, asked for with another digit count
    g.keygen_set([(RELIN, 0)], ekeys[:1], seeds[:1], download=False)
    assert err(lib.evah_key_download_c0(g.h, RELIN, 0, D - 1, p_c0)) == "invalid key digit count"
    g.close()
    # a limb shard holds rows of the keys and no whole secret key
    sh, _, _ = _secret_ctx(N, primes, rng)
    sh.set_shard(1, 2)
    assert kset(sh, *one) == "a limb shard holds no whole secret key"
    assert err(lib.evah_keygen_public(sh.h, p_e, p_s, 1, p_c0)) == "a limb shard holds no whole secret key"
    assert "limb shard" in err(lib.evah_key_download_c0(sh.h, RELIN, 0, D, p_c0))
    assert sh.key_bytes() == 0
    sh.close()
