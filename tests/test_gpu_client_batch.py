"""GPU: the client calls for a batch per call.  evah_encode_encrypt_many / _symmetric_many against the
single calls (evah_pt_encode -> evah_encrypt / evah_encrypt_symmetric), the oracle-built ciphertext and the numpy seed
expansion, word for word; evah_decrypt_decode_many against the oracle's decode and the single call as float64 BIT
PATTERNS; the refusals with the single calls' messages; and the product flow encrypt_batch -> execute_batch ->
decrypt_batch.  Shapes: N = 1024 is below one FFT tile (2048 points), 2048 exactly one, 4096 the smallest two-pass
transform, 65536 the 5 + 11 stage split; batch 8 / 9 are the two ways seeds travel; 70 instances are two groups."""
import numpy as np
import pytest

from eva import evaluate, load, save
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys
from eva_amd import backend, workloads
from oracle import pyoracle as po
from test_gpu_client import _flow
from test_seeded_cpu import expand_limb

pytestmark = pytest.mark.gpu

CHAINS = [(1024, [40, 30, 40, 41]), (2048, [60, 40, 60]), (4096, [60, 20, 60, 60])]
SCALE = 2.0 ** 30


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


class _Env:
    """a context with a random public key and a ternary secret key, and the oracle of the same chain"""

    def __init__(self, N, bits):
        self.N, self.primes = N, po.coeff_modulus_create(N, bits)
        self.k = len(self.primes)
        self.o = po.Oracle(N, self.primes)
        self.g = backend.Context(N, self.primes)
        self.rng = np.random.default_rng(N)
        self.pk = np.stack([self.rand_poly(self.k) for _ in range(2)])
        s = self.rng.integers(-1, 2, size=N)
        self.sk = np.stack([self.o.ntt(i, np.array([int(v) % self.primes[i] for v in s], dtype=np.uint64)) for i in range(self.k)])
        self.g.upload_public_key(self.pk)
        self.g.upload_secret_key(self.sk)

    def rand_poly(self, limbs):
        return np.stack([self.rng.integers(0, self.primes[i], size=self.N, dtype=np.uint64) for i in range(limbs)])

    def small(self, batch):
        r = self.rng
        rows = [np.stack([r.integers(-1, 2, size=self.N), r.integers(-20, 21, size=self.N), r.integers(-20, 21, size=self.N)])
                for _ in range(batch)]
        return np.array(rows, dtype=np.int8).reshape(batch, 3, self.N)   # (also for batch 0, which the refusals pass)

    def oracle_encrypt(self, values, l, small):
        """test_gpu_client.py's oracle-built ciphertext with o.encode as the plaintext"""
        o, primes, N = self.o, self.primes, self.N
        ptd = o.encode(l, np.tile(values, (N // 2) // len(values)), SCALE)
        c = np.zeros((2, l + 1, N), dtype=np.uint64)
        for i in range(l + 1):
            q = primes[i]
            sm = [o.ntt(i, np.array([int(v) % q for v in small[j]], dtype=np.uint64)).astype(object) for j in range(3)]
            for K in range(2):
                c[K, i] = ((self.pk[K, i].astype(object) * sm[0] + sm[1 + K]) % q).astype(np.uint64)
        return o.add_plain(o.rescale(c), ptd)


_ENVS = {}


def _env_of(cfg):
    if cfg[0] not in _ENVS:
        _ENVS[cfg[0]] = _Env(*cfg)
    return _ENVS[cfg[0]]


@pytest.fixture(params=CHAINS, ids=lambda c: f"N{c[0]}")
def env(request):
    return _env_of(request.param)


@pytest.fixture(params=[CHAINS[0], CHAINS[2]], ids=lambda c: f"N{c[0]}")
def dec_env(request):
    """the decrypt cases: every level of the N = 1024 and N = 4096 chains"""
    return _env_of(request.param)


# ---- 1. encode + encrypt, public key

@pytest.mark.parametrize("batch", [1, 3, 64])
def test_encode_encrypt_many_equals_single_calls(env, batch):
    g, N, k = env.g, env.N, env.k
    for n_values in (1, 8, N // 2):
        for l in sorted({1, k - 1}):
            values = env.rng.uniform(-4, 4, (batch, n_values))
            small = env.small(batch)
            ct = g.encode_encrypt_many(values, l, SCALE, small)
            assert ct.batch == batch and ct.info() == (2, l, SCALE)
            got = ct.download().reshape(batch, 2, l, N)   # (a handle of one instance downloads without the batch axis)
            for b in range(batch):
                want = g.encrypt(g.encode_pt(values[b], l, SCALE), small[b]).download()
                assert np.array_equal(ct.unstack(b).download(), want), f"instance {b} (n_values={n_values}, l={l})"
                assert np.array_equal(got[b], want)
            # the single call runs the same device body, so the oracle is the independent reference: every instance at
            # N = 1024, the first and the last of batch 3 at one FFT tile and at the smallest two-pass transform
            for b in range(batch) if N == 1024 else (0, 2) if batch == 3 else ():
                assert np.array_equal(got[b], env.oracle_encrypt(values[b], l, small[b])), f"oracle, instance {b} (n_values={n_values}, l={l})"


def test_encode_encrypt_many_two_pass_5_plus_11():
    e = _Env(65536, [60, 60, 60])
    try:
        values, small = e.rng.uniform(-4, 4, (2, 8)), e.small(2)
        ct = e.g.encode_encrypt_many(values, 2, SCALE, small)
        for b in range(2):
            want = e.g.encrypt(e.g.encode_pt(values[b], 2, SCALE), small[b]).download()
            assert np.array_equal(ct.unstack(b).download(), want), f"instance {b}"
    finally:
        e.g.close()


# ---- 2. encode + encrypt, secret key with one seed per instance

@pytest.mark.parametrize("batch", [8, 9])
def test_encode_encrypt_symmetric_many_equals_single_calls_and_numpy_expansion(env, batch):
    g, N, k = env.g, env.N, env.k
    for n_values in (1, 8, N // 2):
        for l in sorted({1, k - 1}):
            values = env.rng.uniform(-4, 4, (batch, n_values))
            errs = env.rng.integers(-20, 21, size=(batch, N)).astype(np.int8)
            seeds = [env.rng.integers(0, 256, size=32, dtype=np.uint8).tobytes() for _ in range(batch)]
            ct = g.encode_encrypt_symmetric_many(values, l, SCALE, errs, seeds)
            assert ct.batch == batch and ct.info() == (2, l, SCALE)
            for b in range(batch):
                got = ct.unstack(b).download()
                for i in range(l):
                    assert np.array_equal(got[1, i], expand_limb(seeds[b], i, env.primes[i], N)), f"c1 of instance {b}, limb {i}"
                want = g.encrypt_symmetric(g.encode_pt(values[b], l, SCALE), errs[b], seeds[b]).download()
                assert np.array_equal(got[0], want[0]), f"c0 of instance {b} (n_values={n_values}, l={l})"
                assert np.array_equal(got[1], want[1])
            if batch == 9:   # the single call runs the same device body: an oracle-built c0 = encode(v) - (a s + NTT(e))
                for b in (0, batch - 1):
                    m = env.o.encode(l, np.tile(values[b], (N // 2) // n_values), SCALE)
                    for i in range(l):
                        q = env.primes[i]
                        a = expand_limb(seeds[b], i, q, N).astype(object)
                        en = env.o.ntt(i, np.array([int(v) % q for v in errs[b]], dtype=np.uint64)).astype(object)
                        want0 = ((m[i].astype(object) - (a * env.sk[i].astype(object) + en)) % q).astype(np.uint64)
                        assert np.array_equal(ct.unstack(b).download()[0, i], want0), f"oracle c0 of instance {b}, limb {i} (n_values={n_values}, l={l})"


# ---- 3. decrypt + decode

def _known_ct(env, l, size, scale):
    """a ciphertext of an encoded message (test_decode_parity.py): c0 = m - c1 s - c2 s^2 with random c1, c2"""
    o, primes = env.o, env.primes
    m = o.encode(l, env.rng.uniform(-4, 4, env.N // 2), scale)
    ct = np.stack([env.rand_poly(l) for _ in range(size)])
    other = ct.copy()
    other[0] = 0
    rest = o.decrypt(other, env.sk)
    ct[0] = np.stack([(m[i].astype(object) - rest[i].astype(object)) % primes[i] for i in range(l)]).astype(np.uint64)
    return ct


@pytest.mark.parametrize("n", [1, 3, 64])
def test_decrypt_decode_many_returns_the_oracles_doubles(dec_env, n):
    env = dec_env
    g, o, N = env.g, env.o, env.N
    for l in range(1, env.k):
        for size in (2, 3):
            # uniformly random residues (full width, both signs of the composed coefficient), and one encoded message
            data = [np.stack([env.rand_poly(l) for _ in range(size)]) for _ in range(n)]
            if n > 1 or size == 2:   # (a list of one: the encoded message at size 2, random residues at size 3)
                data[-1] = _known_ct(env, l, size, SCALE)
            cts = [g.upload_ct(d, SCALE) for d in data]
            wants = [o.decode(o.decrypt(d, env.sk), SCALE) for d in data]
            for n_out in (1, N // 2):
                got = g.decrypt_decode_many(cts, n_out)
                assert got.shape == (n, n_out)
                for b in range(n):
                    assert _bits_equal(got[b], wants[b][:n_out]), f"oracle: ciphertext {b} (l={l}, size={size}, n_out={n_out})"
                for b in range(n):
                    assert _bits_equal(got[b], g.decrypt_decode(cts[b], n_out)), f"single call: ciphertext {b} (l={l}, size={size}, n_out={n_out})"


def test_decrypt_decode_many_reads_views_in_place_and_caches_tables(env):
    g, o, N, k = env.g, env.o, env.N, env.k
    l = k - 2   # every chain here has at least two data levels
    alone = np.stack([env.rand_poly(l) for _ in range(2)])
    stacked = [np.stack([env.rand_poly(l) for _ in range(2)]) for _ in range(3)]
    above = np.stack([env.rand_poly(l + 1) for _ in range(2)])
    batch = g.stack([g.upload_ct(d, SCALE) for d in stacked])
    switched = g.mod_switch(g.upload_ct(above, SCALE))    # a view with the polynomial stride of l + 1 limbs
    cts = [g.upload_ct(alone, SCALE), batch.unstack(1), switched, batch.unstack(2)]
    data = [alone, stacked[1], above[:, :l], stacked[2]]
    got = g.decrypt_decode_many(cts, N // 2)
    for b in range(4):
        assert _bits_equal(got[b], o.decode(o.decrypt(data[b], env.sk), SCALE)[:N // 2]), f"ciphertext {b}"
        assert _bits_equal(got[b], g.decrypt_decode(cts[b], N // 2))
    # another level of the same context, then the first again: the cached tables of both levels stay right
    top = g.upload_ct(above, SCALE)
    assert _bits_equal(g.decrypt_decode_many([top], 8)[0], o.decode(o.decrypt(above, env.sk), SCALE)[:8])
    assert _bits_equal(g.decrypt_decode_many(cts, 8), got[:, :8])
    assert _bits_equal(g.decrypt_decode_many([top, top], 8)[1], g.decrypt_decode(top, 8))
    # the single entry point on an unstack view and on the mod-switched view, against the oracle's doubles themselves
    for b in (1, 2):
        assert _bits_equal(g.decrypt_decode(cts[b], N // 2), o.decode(o.decrypt(data[b], env.sk), SCALE)[:N // 2]), f"single call, view {b}"


# ---- 4. refusals, with the single calls' messages where one exists

def _err(call, *args):
    with pytest.raises(RuntimeError) as e:
        call(*args)
    return str(e.value)


def test_refusals(env):
    g, N, k = env.g, env.N, env.k
    l = k - 1
    one = lambda b: (env.rng.uniform(-1, 1, (b, 8)), l, SCALE, env.small(b))
    sym = lambda b: (env.rng.uniform(-1, 1, (b, 8)), l, SCALE, np.zeros((b, N), dtype=np.int8), [bytes(32)] * b)
    for b in (0, 65):
        assert "batch must be 1..64" in _err(g.encode_encrypt_many, *one(b))
        assert "batch must be 1..64" in _err(g.encode_encrypt_symmetric_many, *sym(b))
    ct = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), SCALE)
    assert "batch must be 1..64" in _err(g.decrypt_decode_many, [], 8)
    assert "batch must be 1..64" in _err(g.decrypt_decode_many, [ct] * 65, 8)
    # the single calls' checks, message for message
    v, _, _, small = one(2)
    assert _err(g.encode_encrypt_many, v[:, :3], l, SCALE, small) == _err(g.encode_pt, v[0, :3], l, SCALE)
    assert _err(g.encode_encrypt_many, v, k, SCALE, small) == _err(g.encode_pt, v[0], k, SCALE)
    assert _err(g.encode_encrypt_symmetric_many, v, 0, SCALE, small[:, 0], [bytes(32)] * 2) == _err(g.encode_pt, v[0], 0, SCALE)
    assert _err(g.decrypt_decode_many, [ct], 0) == _err(g.decrypt_decode, ct, 0)
    assert _err(g.decrypt_decode_many, [ct], N) == _err(g.decrypt_decode, ct, N)
    # mismatches in the decrypt list are named by argument index
    if l > 1:
        lower = g.mod_switch(ct)
        assert "ciphertext 2: limb count" in _err(g.decrypt_decode_many, [ct, ct, lower], 8)
    other_scale = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), 2.0 * SCALE)
    assert "ciphertext 1: scale" in _err(g.decrypt_decode_many, [ct, other_scale], 8)
    three = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(3)]), SCALE)
    assert "ciphertext 1: size" in _err(g.decrypt_decode_many, [ct, three], 8)
    batched = g.stack([ct, ct])
    msg = _err(g.decrypt_decode_many, [ct, batched], 8)
    assert "ciphertext 1" in msg and "decrypt takes a single ciphertext" in msg
    assert "decrypt takes a single ciphertext" in _err(g.decrypt_decode, batched, 8)
    # a capturing context (one real call is captured around the refusals, so that the graph is an ordinary one)
    g.capture_begin()
    try:
        neg = g.negate(ct)
        cap = [_err(g.encode_encrypt_many, *one(2)), _err(g.encode_encrypt_symmetric_many, *sym(2)), _err(g.decrypt_decode_many, [ct], 8)]
        single = _err(g.decrypt_decode, ct, 8)
    finally:
        g.graph_free(g.capture_end())
    del neg
    assert cap == [single] * 3 and "cannot be captured" in single
    # missing keys
    bare = backend.Context(N, env.primes)
    try:
        ctb = bare.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), SCALE)
        ptb = bare.encode_pt(v[0], l, SCALE)
        assert _err(bare.encode_encrypt_many, *one(2)) == _err(bare.encrypt, ptb, small[0]) == "public key not present"
        assert _err(bare.encode_encrypt_symmetric_many, *sym(2)) == _err(bare.encrypt_symmetric, ptb, small[0, 0], bytes(32)) == "secret key not present"
        assert _err(bare.decrypt_decode_many, [ctb], 8) == _err(bare.decrypt_decode, ctb, 8) == "secret key not present"
    finally:
        bare.close()


# ---- 5. product flow

def _words(val):
    return {n: (val.get(n)[:4], np.asarray(val.get(n)[4])) for n in val.names()}


def _same(a, b):
    wa, wb = _words(a), _words(b)
    assert sorted(wa) == sorted(wb)
    for n in wa:
        assert wa[n][0] == wb[n][0], (n, wa[n][0], wb[n][0])
        assert np.array_equal(wa[n][1], wb[n][1]), f"value {n} differs"


def _flow_case(name):
    if name == "flow4096":
        compiled, params, sig = _flow(512, 4096, 40)
        rng = np.random.default_rng(5)
        xs = [{'x': list(rng.uniform(-2, 2, 512)), 'y': list(rng.uniform(-2, 2, 512))} for _ in range(5)]
    else:
        # Sobel at input scale 2^45, where the compiler itself picks N = 16384 (7 primes, 380 bits).  The 1e-4 below is a
        # bound on CKKS noise, and the example's 2^25 cannot meet it on any path: a fresh encryption is off by about
        # sigma sqrt(N) / scale = 3.2 * 128 / 2^25 ~ 1e-5 per slot, and Sobel amplifies an input error by up to
        # 8 (filter) * 2|Ix| ~ 8 * p'(x) ~ 460 at x = 32, about 3e4: errors of 0.1 and more (test_gpu_configs.py keeps to a
        # mean-square bound for that reason).  At 2^45 the same product is about 3e-7, which leaves the noise of the
        # evaluation's own key switches and rescales two orders of magnitude of room under the bound.
        prog = workloads.sobel(64, 64, 4096)
        prog.set_input_scales(45)
        prog.set_output_ranges(20)
        compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
        assert params.poly_modulus_degree == 16384
        xs = [workloads.image(4096, shift=11 * b) for b in range(3)]
    return compiled, params, sig, xs


@pytest.mark.parametrize("case", ["flow4096", "sobel16384"])
def test_product_flow_batched_client(case, monkeypatch, tmp_path):
    compiled, params, sig, xs = _flow_case(case)
    pub, sec = generate_keys(params, 5)
    refs = [evaluate(compiled, x) for x in xs]

    def flow(encrypt, label):
        """encrypt_batch -> execute_batch -> decrypt_batch; no ciphertext crosses PCIe between the first and the last call"""
        before = pub.transfer_stats()
        encs = encrypt()
        assert all(e.is_resident(n) for e in encs for n in e.names())
        outs = pub.execute_batch(compiled, encs)
        got = sec.decrypt_batch(outs, sig)
        after = pub.transfer_stats()
        assert after["ct_uploads"] == before["ct_uploads"] and after["ct_downloads"] == before["ct_downloads"], (label, before, after)
        assert len(got) == len(xs)
        for b, o in enumerate(outs):
            want = sec.decrypt(o, sig)
            assert sorted(got[b]) == sorted(want) == sorted(refs[b])
            for n in want:
                assert _bits_equal(got[b][n], want[n]), f"{label}: instance {b}, output {n}"
                err = np.abs(np.array(got[b][n]) - np.array(refs[b][n])).max()
                print(f"{case} {label}: instance {b}, output {n}: max error {err:.3g}")
                assert err < 1e-4, (label, b, n)
        return encs, outs

    encs, outs = flow(lambda: pub.encrypt_batch(xs, sig), "public")
    # the same with secret-key encryption: seeded values
    sencs, _ = flow(lambda: sec.encrypt_batch(xs, sig, seed=7), "symmetric")
    _same(sencs[0], sec.encrypt(xs[0], sig, seed=7))
    seeds = [e.seed(n) for e in sencs for n in e.names()]
    assert None not in seeds and len(set(seeds)) == len(seeds)
    # one instance survives save / load as a seeded value with identical words
    path = str(tmp_path / "one.sealvals")
    save(sencs[1], path)
    back = load(path)
    for n in back.names():
        assert back.seed(n) == sencs[1].seed(n) and back.on_host(n)
    _same(back, sencs[1])
    # the host path's words for that seed
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    pub0, sec0 = generate_keys(params, 5)   # same seed: same keys
    hencs = sec0.encrypt_batch(xs, sig, seed=7)
    for d, h in zip(sencs, hencs):
        assert [d.seed(n) for n in sorted(d.names())] == [h.seed(n) for n in sorted(h.names())]
        _same(d, h)
    monkeypatch.delenv("EVA_DEVICE_CLIENT")
    if case != "flow4096":
        return
    # one decrypt_batch list whose values are resident, host words only (uploaded first, as decrypt does) and of another
    # limb count and scale (the first limb of the inputs' words, the same ciphertexts modulo the first prime alone, under
    # the outputs' names): the runs split where the shape changes
    path = str(tmp_path / "out.sealvals")
    save(outs[1], path)
    loaded = load(path)
    assert not any(loaded.is_resident(n) for n in loaded.names())
    hand = type(loaded)()
    for out_name, in_name in (('z', 'x'), ('w', 'y')):
        _, _, _, scale, words = encs[0].get(in_name)
        hand._set_cipher(out_name, words[:, :1], scale)
        assert hand.get(out_name)[2] == 1 != outs[0].get(out_name)[2], "the hand-made value must differ in limb count from the outputs"
    assert hand.get('z')[3] != outs[0].get('z')[3]
    mixed = [outs[0], loaded, hand, outs[2], hand, loaded]
    got = sec.decrypt_batch(mixed, sig)
    for b, v in enumerate(mixed):
        want = sec.decrypt(v, sig)
        assert sorted(got[b]) == sorted(want) == ['w', 'z']
        for n in want:
            assert _bits_equal(got[b][n], want[n]), f"mixed list: value {b}, output {n}"
    for b in (0, 1):
        for n in refs[b]:
            assert np.abs(np.array(got[b][n]) - np.array(refs[b][n])).max() < 1e-4
    for out_name, in_name in (('z', 'x'), ('w', 'y')):
        assert np.abs(np.array(got[2][out_name]) - np.array(xs[0][in_name])).max() < 1e-4


def test_batched_client_with_host_valuations(monkeypatch):
    """EVA_RESIDENT=0: the batched calls download their results as encrypt does (c0 alone for seeded values), and
    decrypt_batch uploads what it is given"""
    compiled, params, sig, xs = _flow_case("flow4096")
    pub, sec = generate_keys(params, 5)
    sencs = sec.encrypt_batch(xs, sig, seed=7)
    monkeypatch.setenv("EVA_RESIDENT", "0")
    pub0, sec0 = generate_keys(params, 5)   # same seed: same keys
    assert not pub0.resident
    hencs = sec0.encrypt_batch(xs, sig, seed=7)
    for d, h in zip(sencs, hencs):
        assert not any(h.is_resident(n) for n in h.names()) and all(h.on_host(n) for n in h.names())
        assert [d.seed(n) for n in sorted(d.names())] == [h.seed(n) for n in sorted(h.names())]
        _same(d, h)
    refs = [evaluate(compiled, x) for x in xs]
    for label, encs in (("public", pub0.encrypt_batch(xs, sig)), ("symmetric", hencs)):
        assert not any(e.is_resident(n) for e in encs for n in e.names()) and all(e.on_host(n) for e in encs for n in e.names())
        back = sec0.decrypt_batch(encs, sig)
        outs = pub0.execute_batch(compiled, encs)
        assert not any(o.is_resident(n) for o in outs for n in o.names())
        got = sec0.decrypt_batch(outs, sig)
        for b in range(len(xs)):
            want_in, want_out = sec0.decrypt(encs[b], sig), sec0.decrypt(outs[b], sig)
            for n in ('x', 'y'):
                assert _bits_equal(back[b][n], want_in[n]), (label, b, n)
                assert np.abs(np.array(back[b][n]) - np.array(xs[b][n])).max() < 1e-4, (label, b, n)
            for n in refs[b]:
                assert _bits_equal(got[b][n], want_out[n]), (label, b, n)
                assert np.abs(np.array(got[b][n]) - np.array(refs[b][n])).max() < 1e-4, (label, b, n)


def test_config4_parameters_decrypt_batch_equals_the_loop():
    """config 4's own parameter set (Sobel at input scale 2^25, 6 primes, N = 2^14), where CKKS noise rules out a tight
    bound against evaluate (see _flow_case): the batched client against the loop of single calls, as bit patterns"""
    compiled, params, sig, _ = workloads.compile_config("c4")
    assert params.poly_modulus_degree == 16384 and len(params.prime_bits) == 6
    pub, sec = generate_keys(params, 5)
    xs = [workloads.image(4096, shift=11 * b) for b in range(3)]
    for encs in (pub.encrypt_batch(xs, sig), sec.encrypt_batch(xs, sig, seed=7)):
        outs = pub.execute_batch(compiled, encs)
        for vals in (encs, outs):
            got = sec.decrypt_batch(vals, sig)
            for b, v in enumerate(vals):
                want = sec.decrypt(v, sig)
                assert sorted(got[b]) == sorted(want)
                for n in want:
                    assert _bits_equal(got[b][n], want[n]), f"instance {b}, value {n}"
    _same(encs[0], sec.encrypt(xs[0], sig, seed=7))


def test_seventy_instances_are_two_groups():
    compiled, params, sig = _flow(8, 1024, 30)
    pub, sec = generate_keys(params, 6)
    rng = np.random.default_rng(8)
    xs = [{'x': list(rng.uniform(-2, 2, 8)), 'y': list(rng.uniform(-2, 2, 8))} for _ in range(70)]
    for encs in (pub.encrypt_batch(xs, sig), sec.encrypt_batch(xs, sig, seed=3)):
        assert len(encs) == 70
        got = sec.decrypt_batch(encs, sig)
        for b in range(70):
            want = sec.decrypt(encs[b], sig)
            for n in ('x', 'y'):
                assert _bits_equal(got[b][n], want[n]), (b, n)
                assert np.abs(np.array(got[b][n]) - np.array(xs[b][n])).max() < 1e-4, (b, n)
    assert len({e.seed(n) for e in encs for n in ('x', 'y')}) == 140
    _same(encs[0], sec.encrypt(xs[0], sig, seed=3))
