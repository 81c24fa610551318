"""GPU: seed-compressed evaluation keys on the MI355X.  evah_key_upload_seeded takes c0 and one
32-byte seed per digit and expands every c1 row — and the radix-2^30 split copy — in one launch (k_key_expand): the
installed words are compared directly (evah_test_key_words) with numpy and with what evah_key_upload installs for the
materialised key, on whole contexts and on limb shards; the key-switching entry points and execute() in every mode
then give the same bits from a seeded upload as from a full one, and the oracle's."""
import os
import subprocess
import sys

import numpy as np
import pytest

from eva import save, load
from eva.ckks import CKKSCompiler, CKKSParameters
from eva.seal import generate_keys, SEALValuation
from eva_amd import backend, workloads
from evatest import oracle_execute
from oracle import pyoracle as po
from test_seeded_cpu import expand_limb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RELIN, GALOIS = backend.KEY_RELIN, backend.KEY_GALOIS


def _ctx(N, primes, **knobs):
    """a context created under the given launch knobs (read once, at creation), as test_gpu_knobs.py sets them"""
    old = {k: os.environ.get(k) for k in knobs}
    os.environ.update({k: str(v) for k, v in knobs.items()})
    try:
        return backend.Context(N, primes)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_KEYS = {}


def _compressed(N, bits, steps=()):
    """(primes, {0: (c0, seeds, words), elt: ...}) of a compressed key pair: c0 [D][k][N], seeds [D][32], and the
    host's materialised words [D][2][k][N]; made once per shape"""
    tag = (N, tuple(bits), tuple(steps))
    if tag not in _KEYS:
        pub, _ = generate_keys(CKKSParameters(list(bits), set(steps), N), 7, compress_keys=True)
        seeds = pub.key_seeds()
        words = {0: pub.relin_key()}
        words.update(pub.galois_keys())
        _KEYS[tag] = (pub.primes, {e: (np.ascontiguousarray(w[:, 0]), seeds[e], w) for e, w in words.items()})
    return _KEYS[tag]


def _split(x):
    return (x & np.uint64(0x3FFFFFFF)) | ((x >> np.uint64(30)) << np.uint64(32))


def _numpy_words(c0, seeds, primes, N):
    out = np.empty((c0.shape[0], 2) + c0.shape[1:], dtype=np.uint64)
    out[:, 0] = c0
    for J in range(c0.shape[0]):
        for i, q in enumerate(primes):
            out[J, 1, i] = expand_limb(seeds[J].tobytes(), i, q, N)
    return out


def _upload(g, elt, c0, seeds):
    if elt == 0:
        g.upload_relin_key_seeded(c0, seeds)
    else:
        g.upload_galois_key_seeded(elt, c0, seeds)


def _upload_full(g, elt, words):
    if elt == 0:
        g.upload_relin_key(words)
    else:
        g.upload_galois_key(elt, words)


LAYOUTS = [
    # mixed sizes.  Primes below 2^54 need no top-bit shape for the radix-2^30 inner product (evah_ctx_create: all_tb), so
    # this chain HAS a split copy, from the full upload as from the seeded one; a chain that has none for its primes'
    # sake needs a prime of 2^54 or more that is far from a power of two: test_no_split_copy_for_a_prime_of_another_shape
    (1024, [60, 30, 45, 50, 33, 60], (1, -3), True),
    (2048, [60, 50, 50, 60], (5,), True),                # top-bit: the split copy comes out of the same launch
    (1 << 16, [60] + [50] * 9 + [60], (), True),         # relinearization key only
    (1024, [30] * 16 + [31, 31], (2,), True),            # 17 digits: the seeds travel as a device buffer
]


@pytest.mark.parametrize("N,bits,steps,has_split", LAYOUTS, ids=["N1024_mixed", "N2048_topbit", "N65536_relin", "N1024_17digits"])
def test_installed_words_match_numpy_and_the_full_upload(N, bits, steps, has_split):
    primes, keys = _compressed(N, bits, steps)
    D = len(primes) - 1
    g, f = backend.Context(N, primes), backend.Context(N, primes)
    for elt, (c0, seeds, words) in keys.items():
        kind = RELIN if elt == 0 else GALOIS
        _upload(g, elt, c0, seeds)
        _upload_full(f, elt, words)
        got = g.key_words(kind, elt, 0, D)
        want = _numpy_words(c0, seeds, primes, N)
        assert np.array_equal(got[:, 0], c0), f"key {elt}: c0 as given"
        assert np.array_equal(got, want), f"key {elt}: c1 against the numpy expansion"
        assert np.array_equal(want, words), f"key {elt}: the host's materialised words"
        assert np.array_equal(got, f.key_words(kind, elt, 0, D)), f"key {elt}: seeded against full upload"
        if has_split:
            sp = g.key_words(kind, elt, 1, D)
            assert np.array_equal(sp, _split(want)), f"key {elt}: split copy"
            assert np.array_equal(sp, f.key_words(kind, elt, 1, D)), f"key {elt}: split copy against the full upload's"
        else:
            for x in (g, f):
                with pytest.raises(backend.EvaHipError, match="no split copy"):
                    x.key_words(kind, elt, 1, D)
    assert g.key_bytes() == f.key_bytes() == len(keys) * D * 2 * len(primes) * N * 8
    assert g.key_bytes_detail() == f.key_bytes_detail()
    # a second upload replaces the key (and its split copy) in place
    c0, seeds, words = keys[0]
    _upload(g, 0, c0[::-1].copy(), seeds)
    assert np.array_equal(g.key_words(RELIN, 0, 0, D)[:, 0], c0[::-1])
    assert g.key_bytes() == f.key_bytes()
    g.close()
    f.close()


def test_no_split_copy_for_a_prime_of_another_shape():
    """a chain that is not all top-bit: a 55-bit prime 2^53 away from 2^55 (no generated prime is like that, so the key is
    made here: random c0, random seeds).  Neither upload keeps a split copy, and the words are the numpy expansion's"""
    from eva_amd.hostref import _is_prime, coeff_modulus_create
    N = 1024
    q = 3 * (1 << 53) + 1
    while not _is_prime(q):
        q += 2 * N
    assert q.bit_length() == 55 and (1 << 55) - q > (1 << 32)
    base = coeff_modulus_create(N, [60, 30, 45, 60])
    primes = [base[0], q, base[1], base[2], base[3]]
    k, D = len(primes), len(primes) - 1
    rng = np.random.default_rng(55)
    c0 = np.stack([rng.integers(0, p, size=(D, N), dtype=np.uint64) for p in primes], axis=1)
    seeds = rng.integers(0, 256, size=(D, 32), dtype=np.uint8)
    words = _numpy_words(c0, seeds, primes, N)
    g, f = backend.Context(N, primes), backend.Context(N, primes)
    g.upload_relin_key_seeded(c0, seeds)
    f.upload_relin_key(words)
    assert np.array_equal(g.key_words(RELIN, 0, 0), words)
    assert np.array_equal(f.key_words(RELIN, 0, 0), words)
    for x in (g, f):
        with pytest.raises(backend.EvaHipError, match="no split copy"):
            x.key_words(RELIN, 0, 1)
    assert g.key_bytes_detail() == f.key_bytes_detail() == (D * 2 * k * N * 8, 0, 0)
    g.close()
    f.close()


def test_no_split_copy_without_mac3():
    N, bits, steps, _ = LAYOUTS[1]
    primes, keys = _compressed(N, bits, steps)
    g = _ctx(N, primes, EVAH_MAC3=0)
    c0, seeds, words = keys[0]
    g.upload_relin_key_seeded(c0, seeds)
    assert np.array_equal(g.key_words(RELIN, 0, 0), words)
    with pytest.raises(backend.EvaHipError, match="no split copy"):
        g.key_words(RELIN, 0, 1)
    g.close()


@pytest.mark.parametrize("G", [2, 3])
def test_limb_shards_keep_and_expand_their_own_rows(G):
    """k - 1 = 5 data limbs: not a multiple of 2 or 3, so the shards hold different row counts"""
    N, bits, steps, _ = LAYOUTS[0]
    primes, keys = _compressed(N, bits, steps)
    k, D = len(primes), len(primes) - 1
    for s in range(G):
        g, f = backend.Context(N, primes), backend.Context(N, primes)
        g.set_shard(s, G)
        f.set_shard(s, G)
        rows = list(range(s, k - 1, G)) + [k - 1]
        for elt, (c0, seeds, words) in keys.items():
            kind = RELIN if elt == 0 else GALOIS
            _upload(g, elt, c0, seeds)
            _upload_full(f, elt, words)
            got = g.key_words(kind, elt, 0, D)
            assert got.shape == (D, 2, len(rows), N)
            assert np.array_equal(got, words[:, :, rows]), f"shard {s} of {G}, key {elt}"
            assert np.array_equal(got, f.key_words(kind, elt, 0, D))
            with pytest.raises(backend.EvaHipError, match="no split copy"):
                g.key_words(kind, elt, 1, D)
        assert g.key_bytes() == f.key_bytes() == len(keys) * D * 2 * len(rows) * N * 8
        g.close()
        f.close()


def _ops_check(mac3=1):
    """relinearize, rotate, a hoisted rotation set and the chain step on a seeded-upload context, a full-upload context
    of the same materialised keys, and the oracle: the same bits.  One all-top-bit chain (the split copy is what the
    inner products read unless EVAH_MAC3=0) and one with small primes."""
    steps = [1, 5, -3]
    for N, bits in [(2048, [60, 50, 50, 50, 60]), (1024, [60, 30, 45, 50, 33, 60])]:
        primes, keys = _compressed(N, bits, steps)
        k, l = len(primes), len(primes) - 1
        o = po.Oracle(N, primes)
        g = _ctx(N, primes, EVAH_HOIST_MIN_TILES=0, EVAH_MAC3=mac3)
        f = _ctx(N, primes, EVAH_HOIST_MIN_TILES=0, EVAH_MAC3=mac3)
        elts = {st: g.galois_elt_from_step(st) for st in steps}
        assert sorted(keys) == sorted([0] + list(elts.values()))
        for elt, (c0, seeds, words) in keys.items():
            _upload(g, elt, c0, seeds)
            _upload_full(f, elt, words)
        rk = keys[0][2]
        gk = {st: keys[elts[st]][2] for st in steps}
        rng = np.random.default_rng(N + mac3)

        def rand(size, nl):
            return np.stack([rng.integers(0, primes[i], size=(size, N), dtype=np.uint64) for i in range(nl)], axis=1)
        a, b, a3 = rand(2, l), rand(2, l), rand(3, l)
        div = bits[-2]

        def both(call):
            x, y = call(g), call(f)
            assert len(x) == len(y)
            for u, v in zip(x, y):
                assert np.array_equal(u, v), "seeded-upload and full-upload contexts differ"
            return x
        up = lambda c, x: c.upload_ct(x, 2.0 ** 30)
        got = both(lambda c: [c.relinearize(up(c, a3)).download()])
        assert np.array_equal(got[0], o.relinearize(a3, rk)), "relinearize"
        got = both(lambda c: [c.rotate(up(c, a), 5).download()])
        assert np.array_equal(got[0], o.rotate(a, 5, gk[5])), "rotate"
        got = both(lambda c: [r.download() for r in c.rotate_many(up(c, a), steps)])
        for st, r in zip(steps, got):
            assert np.array_equal(r, o.rotate(a, st, gk[st])), f"hoisted rotate_many, step {st}"
        got = both(lambda c: [c.multiply_rescale_relinearize(up(c, a), up(c, b), div).download()])
        assert np.array_equal(got[0], o.relinearize(o.rescale(o.multiply(a, b)), rk)), "multiply_rescale_relinearize"
        assert g.key_bytes_detail() == f.key_bytes_detail()   # the permuted copies of the hoisted set included
        g.close()
        f.close()


def test_key_switching_ops_are_bit_identical():
    _ops_check(1)


def test_key_switching_ops_are_bit_identical_without_mac3():
    """EVAH_MAC3=0 in a process of its own"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "tests")]), EVAH_MAC3="0")
    out = subprocess.run([sys.executable, "-c", "import test_gpu_seeded_keys as t; t._ops_check(0); print('ops ok')"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ops ok" in out.stdout, out.stderr[-2000:]


# ---- through the public surface

def _readme():
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(workloads.readme_polynomial())
    return compiled, params, sig, {"x": [i / 1024.0 for i in range(1024)]}


def _sobel():
    prog = workloads.sobel(32, 32, 1024)
    prog.set_input_scales(25)
    prog.set_output_ranges(10)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    return compiled, params, sig, workloads.image(1024)


_WORK = {}


def _work(name, tmp_path_factory):
    """per workload, once: the compiled program, the input ciphertexts as host words (secret-key encryption under a
    fixed seed: the same words for every key pair of test seed 7), the oracle's outputs under the materialised keys,
    and the compressed context saved with format="seal" (the same keys, expanded)"""
    if name not in _WORK:
        compiled, params, sig, inputs = {"readme": _readme, "sobel": _sobel}[name]()
        pub, sec = generate_keys(params, 7, compress_keys=True)
        assert pub.keys_compressed
        enc = sec.encrypt(inputs, sig, seed=11)
        words = [{n: (enc.get(n)[4], enc.get(n)[3]) for n in enc.names()}]
        enc2 = sec.encrypt({n: list(reversed(v)) for n, v in inputs.items()}, sig, seed=12)
        words.append({n: (enc2.get(n)[4], enc2.get(n)[3]) for n in enc2.names()})
        want = [oracle_execute(pub, compiled, _valuation(w)) for w in words]
        path = str(tmp_path_factory.mktemp(name) / "ctx.seal")
        save(pub, path, format="seal")
        _WORK[name] = (compiled, params, words, want, path)
    return _WORK[name]


def _valuation(words):
    v = SEALValuation()
    for n, (data, scale) in words.items():
        v._set_cipher(n, data, scale)
    return v


def _same(a, b):
    assert sorted(a.names()) == sorted(b.names())
    for n in a.names():
        x, y = a.get(n), b.get(n)
        assert x[:4] == y[:4], (n, x[:4], y[:4])
        assert np.array_equal(np.asarray(x[4]), np.asarray(y[4])), f"output {n} differs"


@pytest.mark.parametrize("mode", ["resident", "host", "subdag", "limb", "batch"])
@pytest.mark.parametrize("name", ["readme", "sobel"])
def test_execute_with_compressed_keys_is_bit_exact(name, mode, monkeypatch, tmp_path_factory):
    if mode == "host":
        monkeypatch.setenv("EVA_RESIDENT", "0")
    compiled, params, words, want, seal_path = _work(name, tmp_path_factory)
    kw = {"devices": [0, 0], "shard": mode} if mode in ("subdag", "limb") else {}
    pub, _ = generate_keys(params, 7, compress_keys=True, **kw)
    full = load(seal_path)   # the same keys, kept and uploaded in full
    assert pub.keys_compressed and not full.keys_compressed
    if kw:
        full.devices, full.shard_mode = [0, 0], mode
    if mode == "batch":
        vals = [_valuation(w) for w in words]
        outs, outs_full = pub.execute_batch(compiled, vals), full.execute_batch(compiled, vals)
        for got, ref, oracle in zip(outs, outs_full, want):
            _same(got, oracle)
            _same(got, ref)
        return
    for call in range(3):   # eager walk, plan capture, replay
        got = pub.execute(compiled, _valuation(words[0]))
        _same(got, want[0])
    _same(got, full.execute(compiled, _valuation(words[0])))
    # the device holds exactly the bytes a full upload leaves there
    assert pub.key_bytes() == full.key_bytes()


# ---- argument errors

def test_argument_errors_match_the_full_uploads():
    N, bits, steps, _ = LAYOUTS[0]
    primes, keys = _compressed(N, bits, steps)
    D = len(primes) - 1
    c0, seeds, words = keys[0]
    lib = backend.load()
    g = backend.Context(N, primes)
    u8p = backend.C.POINTER(backend.C.c_uint8)
    p_c0, p_words, p_seeds = backend._p(c0), backend._p(words), seeds.ctypes.data_as(u8p)

    def err(rc):
        assert rc != 0
        return lib.evah_last_error().decode()
    # an even Galois element, an element >= 2 N
    for elt in (4, 2 * N + 1):
        seeded = err(lib.evah_key_upload_seeded(g.h, GALOIS, elt, D, p_c0, p_seeds))
        assert seeded == err(lib.evah_key_upload(g.h, GALOIS, elt, D, p_words)) == "Galois element is not valid"
    # zero digits, more digits than data primes
    for d in (0, D + 1):
        seeded = err(lib.evah_key_upload_seeded(g.h, RELIN, 0, d, p_c0, p_seeds))
        assert seeded == err(lib.evah_key_upload(g.h, RELIN, 0, d, p_words)) == "invalid key digit count"
    assert "unknown key kind" in err(lib.evah_key_upload_seeded(g.h, 7, 0, D, p_c0, p_seeds))
    assert "seed pointer is null" in err(lib.evah_key_upload_seeded(g.h, RELIN, 0, D, p_c0, None))
    assert "key pointer is null" in err(lib.evah_key_upload_seeded(g.h, RELIN, 0, D, None, p_seeds))
    # nothing above installed a key
    assert g.key_bytes() == 0
    with pytest.raises(backend.EvaHipError, match="no such key"):
        g.key_words(RELIN, 0, 0)
    # a shard map that changed between uploads: whole keys first, then the context becomes a limb shard
    g.upload_relin_key_seeded(c0, seeds)
    g.set_shard(1, 2)
    seeded = err(lib.evah_key_upload_seeded(g.h, RELIN, 0, D, p_c0, p_seeds))
    assert seeded == err(lib.evah_key_upload(g.h, RELIN, 0, D, p_words))
    assert "different shard map" in seeded
    g.close()
