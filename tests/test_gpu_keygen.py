"""GPU: evaluation keys generated on the MI355X.  evah_keygen_switch forms c0 = -(a s + NTT(e)) +
[row J] (P mod q_J) s' of every digit in one launch (k_keygen_switch) from the resident secret key, the caller's int8
errors and the seeds a is expanded from.  The keys are compared word for word with the host generator's for the same
draws, checked against the key equation in Python integers without the host generator, compared as installed (words,
split copy, bytes) with an upload of the same c0 + seeds, used by the key-switching entry points against the oracle,
and driven through generate_keys(..., device_keygen=True) and execute() in every mode."""
import numpy as np
import pytest

from eva import save, load
from eva.ckks import CKKSParameters
from eva.seal import generate_keys
from eva_amd import backend
from oracle import pyoracle as po
from test_seeded_cpu import expand_limb
from test_gpu_seeded_keys import _ctx, _numpy_words, _split, _upload, _work, _valuation, _same

pytestmark = pytest.mark.gpu

RELIN, GALOIS = backend.KEY_RELIN, backend.KEY_GALOIS

# the smallest shapes that reach every branch of the kernel and its launch
SHAPES = {
    "N1024_mixed": (1024, [60, 30, 45, 50, 33, 60], (1, -3, 0)),   # mixed prime sizes, a split copy; step 0 = conjugation (2N - 1)
    "N2048_topbit": (2048, [60, 50, 50, 60], (5,)),                # all top-bit, blockIdx.x > 0
    "N1024_17digits": (1024, [30] * 16 + [31, 31], (2,)),          # 17 digits: the seeds travel as a device buffer
}


def _keys(pub):
    out = {0: pub.relin_key()}
    out.update(pub.galois_keys())
    return out


# ---- 1. device keygen equals host keygen

@pytest.mark.parametrize("name", list(SHAPES))
def test_device_keygen_equals_host_keygen(name, tmp_path):
    N, bits, steps = SHAPES[name]
    p = CKKSParameters(list(bits), set(steps), N)
    pubd, secd = generate_keys(p, 7, device_keygen=True)
    pubh, sech = generate_keys(p, 7, compress_keys=True)
    assert pubd.keys_compressed and pubh.keys_compressed
    sd, sh = pubd.key_seeds(), pubh.key_seeds()
    assert sorted(sd) == sorted(sh) and len(sd) == 1 + len(steps)
    assert 2 * N - 1 in sd or 0 not in steps
    for e in sh:
        assert np.array_equal(sd[e], sh[e]), f"seeds of key {e}"
    kd, kh = _keys(pubd), _keys(pubh)
    for e in kh:
        assert np.array_equal(kd[e][:, 0], kh[e][:, 0]), f"c0 of key {e}"
        assert np.array_equal(kd[e], kh[e]), f"materialised words of key {e}"
    assert np.array_equal(secd._secret_key_ntt(), sech._secret_key_ntt())
    assert np.array_equal(pubd.public_key(), pubh.public_key())
    fd, fh = tmp_path / "d.sealpub", tmp_path / "h.sealpub"
    save(pubd, str(fd))
    save(pubh, str(fh))
    assert fd.read_bytes() == fh.read_bytes()
    # the single-device default: the keys are on the device already, and only the draws went up and c0 came down
    k, D = len(pubd.primes), len(pubd.primes) - 1
    assert pubd.key_bytes() == [len(kh) * D * 2 * k * N * 8] and pubh.key_bytes() == [0]
    st = pubd.transfer_stats()
    assert st["h2d_bytes"] == len(kh) * D * (N + 32) and st["d2h_bytes"] == len(kh) * D * k * N * 8


# ---- 2. the key equation, independently of the host generator

def _secret(o, rng):
    """a ternary secret: coefficients, and [k][N] NTT form under every chain prime"""
    s = rng.integers(-1, 2, size=o.N)
    return s, np.stack([o.ntt(i, np.array([int(v) % q for v in s], dtype=np.uint64)) for i, q in enumerate(o.primes)])


def _automorphism(s, elt, N):
    """coefficients of s(X^elt) in Z[X] / (X^N + 1)"""
    out = np.zeros(N, dtype=np.int64)
    for j in range(N):
        m = (j * elt) % (2 * N)
        if m < N:
            out[m] += s[j]
        else:
            out[m - N] -= s[j]
    return out


def test_key_equation_in_python_integers():
    N, bits, _ = SHAPES["N1024_mixed"]
    primes = po.coeff_modulus_create(N, bits)
    k, D = len(primes), len(primes) - 1
    o = po.Oracle(N, primes)
    rng = np.random.default_rng(15)
    s, s_ntt = _secret(o, rng)
    P = primes[-1]
    g = backend.Context(N, primes)
    g.upload_secret_key(s_ntt)
    elt3 = g.galois_elt_from_step(3)
    for kind, elt in [(RELIN, 0), (GALOIS, elt3), (GALOIS, 2 * N - 1)]:
        seeds = rng.integers(0, 256, size=(D, 32), dtype=np.uint8)
        errors = rng.integers(-21, 22, size=(D, N)).astype(np.int8)
        errors[D - 1, 5], errors[D - 1, 6], errors[D - 1, N - 1] = -128, 127, -128   # the ends of the int8 range
        c0 = g.keygen_switch(kind, elt, errors, seeds, install=False)
        assert c0.shape == (D, k, N)
        if kind == GALOIS:
            sp = _automorphism(s, elt, N)
        for i, q in enumerate(primes):
            si = [int(v) for v in s_ntt[i]]
            if kind == RELIN:
                spi = [v * v % q for v in si]
            else:
                spi = [int(v) for v in o.ntt(i, np.array([int(v) % q for v in sp], dtype=np.uint64))]
            for J in range(D):
                c1 = expand_limb(seeds[J].tobytes(), i, q, N)
                f = P % q if i == J else 0
                m = [(int(b) + int(a) * sv - f * spv) % q for b, a, sv, spv in zip(c0[J, i], c1, si, spi)]
                got = o.intt(i, np.array(m, dtype=np.uint64))
                want = np.array([(-int(e)) % q for e in errors[J]], dtype=np.uint64)
                assert np.array_equal(got, want), f"kind {kind}, element {elt}, digit {J}, prime {i}"
    assert g.key_bytes() == 0
    g.close()


# ---- 3. installed layouts

def _draws(rng, D, N):
    return rng.integers(-21, 22, size=(D, N)).astype(np.int8), rng.integers(0, 256, size=(D, 32), dtype=np.uint8)


def _secret_ctx(N, primes, rng, **knobs):
    o = po.Oracle(N, primes)
    _, s_ntt = _secret(o, rng)
    g = _ctx(N, primes, **knobs)
    g.upload_secret_key(s_ntt)
    return g


@pytest.mark.parametrize("name", list(SHAPES))
def test_installed_layouts_match_a_seeded_upload(name):
    N, bits, steps = SHAPES[name]
    primes = po.coeff_modulus_create(N, bits)
    k, D = len(primes), len(primes) - 1
    rng = np.random.default_rng(N + k)
    g, f = _secret_ctx(N, primes, rng), backend.Context(N, primes)
    assert g.key_bytes() == 0
    elts = [0] + [g.galois_elt_from_step(st) if st else 2 * N - 1 for st in steps]
    for elt in elts:
        kind = RELIN if elt == 0 else GALOIS
        errors, seeds = _draws(rng, D, N)
        assert np.array_equal(g.keygen_switch(kind, elt, errors, seeds, install=False), g.keygen_switch(kind, elt, errors, seeds, install=False))
        assert g.key_bytes() == f.key_bytes(), "install=False leaves no key behind"
        c0 = g.keygen_switch(kind, elt, errors, seeds)
        want = _numpy_words(c0, seeds, primes, N)
        got = g.key_words(kind, elt, 0, D)
        assert np.array_equal(got[:, 0], c0), f"key {elt}: the returned c0 is the installed c0"
        assert np.array_equal(got, want), f"key {elt}: c1 against the numpy expansion"
        _upload(f, elt, c0, seeds)
        assert np.array_equal(got, f.key_words(kind, elt, 0, D)), f"key {elt}: against the seeded upload"
        sp = g.key_words(kind, elt, 1, D)
        assert np.array_equal(sp, _split(want)), f"key {elt}: split copy"
        assert np.array_equal(sp, f.key_words(kind, elt, 1, D)), f"key {elt}: split copy against the seeded upload's"
    assert g.key_bytes() == f.key_bytes() == len(elts) * D * 2 * k * N * 8
    assert g.key_bytes_detail() == f.key_bytes_detail()
    # a second generation replaces the key (and its split copy) in place
    for elt in (0, elts[-1]):
        kind = RELIN if elt == 0 else GALOIS
        errors, seeds = _draws(rng, D, N)
        before = g.key_words(kind, elt, 0, D)
        c0 = g.keygen_switch(kind, elt, errors, seeds)
        after = g.key_words(kind, elt, 0, D)
        assert np.array_equal(after, _numpy_words(c0, seeds, primes, N)) and not np.array_equal(after, before)
        assert np.array_equal(g.key_words(kind, elt, 1, D), _split(after))
    assert g.key_bytes_detail() == f.key_bytes_detail()
    g.close()
    f.close()


def test_no_split_copy_without_mac3():
    N, bits, _ = SHAPES["N2048_topbit"]
    primes = po.coeff_modulus_create(N, bits)
    D = len(primes) - 1
    rng = np.random.default_rng(3)
    g = _secret_ctx(N, primes, rng, EVAH_MAC3=0)
    errors, seeds = _draws(rng, D, N)
    c0 = g.keygen_switch(RELIN, 0, errors, seeds)
    assert np.array_equal(g.key_words(RELIN, 0, 0), _numpy_words(c0, seeds, primes, N))
    with pytest.raises(backend.EvaHipError, match="no split copy"):
        g.key_words(RELIN, 0, 1)
    assert g.key_bytes_detail() == (D * 2 * len(primes) * N * 8, 0, 0)
    g.close()


# ---- 4. the keys work

def test_generated_keys_switch_like_uploaded_ones():
    """relinearize, rotate, a hoisted rotation set and the chain step on a context g whose keys were generated in place
    (from draws made here, under the host generator's secret key), a context f that uploaded the materialised words
    [c0, expand(seeds)] of those same keys with evah_key_upload, and the oracle under those words: the same bits (the
    pattern and the two chains of test_gpu_seeded_keys._ops_check).  That the device's words equal the host generator's
    for the host's draws is test_device_keygen_equals_host_keygen."""
    steps = [1, 5, -3]
    for N, bits in [(2048, [60, 50, 50, 50, 60]), (1024, [60, 30, 45, 50, 33, 60])]:
        pub, sec = generate_keys(CKKSParameters(list(bits), set(steps), N), 7, compress_keys=True)
        primes, seeds, words = pub.primes, pub.key_seeds(), _keys(pub)
        k, l = len(primes), len(primes) - 1
        o = po.Oracle(N, primes)
        g = _ctx(N, primes, EVAH_HOIST_MIN_TILES=0)
        f = _ctx(N, primes, EVAH_HOIST_MIN_TILES=0)
        g.upload_secret_key(sec._secret_key_ntt())
        elts = {st: g.galois_elt_from_step(st) for st in steps}
        assert sorted(words) == sorted([0] + list(elts.values()))
        rng = np.random.default_rng(N)
        own = {}
        for elt, w in words.items():
            errors, sd = _draws(rng, l, N)   # keys of its own draws under the same secret: valid keys, other words
            c0 = g.keygen_switch(RELIN if elt == 0 else GALOIS, elt, errors, sd)
            own[elt] = _numpy_words(c0, sd, primes, N)
            assert not np.array_equal(own[elt], w)
            (f.upload_relin_key(own[elt]) if elt == 0 else f.upload_galois_key(elt, own[elt]))
        assert g.key_upload_stats() == (0, 0) and f.key_upload_stats() == (len(words), sum(w.nbytes for w in own.values()))
        rk, gk = own[0], {st: own[elts[st]] for st in steps}

        def rand(size, nl):
            return np.stack([rng.integers(0, primes[i], size=(size, N), dtype=np.uint64) for i in range(nl)], axis=1)
        a, b, a3 = rand(2, l), rand(2, l), rand(3, l)
        div = bits[-2]

        def both(call):
            x, y = call(g), call(f)
            assert len(x) == len(y)
            for u, v in zip(x, y):
                assert np.array_equal(u, v), "generated-in-place and uploaded contexts differ"
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


def test_generated_host_draw_keys_decrypt_a_rotation():
    """the Galois key is a key FOR the rotation: with the host generator's draws (same words as the host's key, test 1)
    the oracle's rotation of a fresh encryption decrypts to the rotated message — the permutation table is the right one"""
    N, bits = 1024, [60, 30, 45, 50, 33, 60]
    pub, sec = generate_keys(CKKSParameters(list(bits), {1}, N), 7, device_keygen=True)
    primes = pub.primes
    o = po.Oracle(N, primes)
    l = len(primes) - 1
    elt = po.galois_elt_from_step(N, 1)
    gk = pub.galois_keys()[elt]
    sk = sec._secret_key_ntt()
    rng = np.random.default_rng(8)
    # an encryption of m under s with zero noise: c1 uniform, c0 = m - c1 s
    m = rng.integers(0, 1 << 20, size=N).astype(np.uint64)
    c1 = np.stack([rng.integers(0, primes[i], size=N, dtype=np.uint64) for i in range(l)])
    c0 = np.empty_like(c1)
    for i in range(l):
        q = primes[i]
        mi = o.ntt(i, m % np.uint64(q))
        c0[i] = np.array([(int(x) - int(a) * int(s)) % q for x, a, s in zip(mi, c1[i], sk[i])], dtype=np.uint64)
    rot = o.rotate(np.stack([c0, c1]), 1, gk)
    want = _automorphism(m.astype(np.int64), elt, N)   # m(X^elt), in the coefficient domain: no permutation table involved
    for i in range(l):
        q = primes[i]
        dec = np.array([(int(x) + int(a) * int(s)) % q for x, a, s in zip(rot[0, i], rot[1, i], sk[i])], dtype=np.uint64)
        diff = [(int(x) - int(y)) % q for x, y in zip(o.intt(i, dec), want)]
        # key-switching noise alone: every digit is below its prime <= 2^60 and multiplies an error of at most 21 per
        # coefficient, summed over N coefficients and D = 5 digits and divided by P > 2^59: below 2 * 1024 * 5 * 21 < 2^18
        assert max(min(v, q - v) for v in diff) < 1 << 18, f"limb {i}"


# ---- 5. public surface

@pytest.mark.parametrize("mode", ["resident", "subdag", "limb", "batch"])
@pytest.mark.parametrize("name", ["readme", "sobel"])
def test_execute_with_device_generated_keys_is_bit_exact(name, mode, tmp_path, tmp_path_factory):
    compiled, params, words, want, _ = _work(name, tmp_path_factory)
    kw = {"devices": [0, 0], "shard": mode} if mode in ("subdag", "limb") else {}
    pub, _ = generate_keys(params, 7, device_keygen=True, **kw)
    ref, _ = generate_keys(params, 7, compress_keys=True, **kw)
    assert pub.keys_compressed and ref.keys_compressed
    N, k = pub.poly_modulus_degree, len(pub.primes)
    whole = (1 + len(pub.galois_keys())) * (k - 1) * 2 * k * N * 8
    if mode == "batch":
        vals = [_valuation(w) for w in words]
        for got, r, oracle in zip(pub.execute_batch(compiled, vals), ref.execute_batch(compiled, vals), want):
            _same(got, oracle)
            _same(got, r)
        return
    # default mode: installed as generated; every other mode: the members and shards upload from the host's c0 + seeds
    assert pub.key_bytes() == ([whole] if mode == "resident" else [0])
    assert pub.key_upload_stats() == {"uploads": 0, "bytes": 0} == ref.key_upload_stats()
    before = pub.transfer_stats()
    got = pub.execute(compiled, _valuation(words[0]))   # eager walk
    first = pub.transfer_stats()
    up_first = pub.key_upload_stats()
    _same(got, want[0])
    for call in range(2):   # plan capture, replay
        got = pub.execute(compiled, _valuation(words[0]))
        _same(got, want[0])
    ref_before = ref.transfer_stats()
    _same(got, ref.execute(compiled, _valuation(words[0])))
    ref_first = ref.transfer_stats()
    if mode == "resident":
        # no key crossed PCIe in the first execute() — nor in any later one — of the pair whose keys were generated in
        # place, while the host-generated pair uploaded every key once, compressed: c0 + 32 bytes per digit
        n_keys = 1 + len(pub.galois_keys())
        assert up_first == {"uploads": 0, "bytes": 0} == pub.key_upload_stats()
        assert ref.key_upload_stats() == {"uploads": n_keys, "bytes": whole // 2 + n_keys * (k - 1) * 32}
        # what the first execute() did send up is its inputs and constants: at least the input words, and byte for byte
        # what the reference pair's first execute() counts for them (transfer_stats counts values, not keys)
        inputs = sum(np.asarray(d).nbytes for d, _ in words[0].values())
        sent = first["h2d_bytes"] - before["h2d_bytes"]
        assert sent >= inputs and sent == ref_first["h2d_bytes"] - ref_before["h2d_bytes"]
        assert pub.key_bytes() == [whole] == ref.key_bytes()
        # save -> load: an ordinary compressed context, which uploads its keys and computes the same bits
        path = str(tmp_path / "ctx.sealpub")
        save(pub, path)
        back = load(path)
        assert back.keys_compressed
        _same(back.execute(compiled, _valuation(words[0])), want[0])
        assert back.key_upload_stats()["uploads"] == n_keys
    else:
        # the key pair's own device state keeps no evaluation key of its own making: the members and shards uploaded
        # theirs from the host's c0 + seeds, exactly as the host-generated pair's did
        assert pub.key_bytes() == ref.key_bytes() and pub.key_upload_stats() == ref.key_upload_stats()


# ---- 6. argument errors

def test_argument_errors():
    """every refusal with its message, none leaving a key behind.  (One refusal cannot be reached through the C ABI: a
    context only exists for a power-of-two N >= 1024, so "N not divisible by 256" never arises.)"""
    N, bits, _ = SHAPES["N1024_mixed"]
    primes = po.coeff_modulus_create(N, bits)
    D = len(primes) - 1
    rng = np.random.default_rng(2)
    lib = backend.load()
    i8p, u8p = backend.C.POINTER(backend.C.c_int8), backend.C.POINTER(backend.C.c_uint8)
    errors, seeds = _draws(rng, D, N)
    c0 = np.zeros((D, len(primes), N), dtype=np.uint64)
    p_e, p_s, p_c0 = errors.ctypes.data_as(i8p), seeds.ctypes.data_as(u8p), backend._p(c0)

    def err(rc):
        assert rc != 0
        return lib.evah_last_error().decode()
    # no secret key on the context: evah_encrypt_symmetric's message
    bare = backend.Context(N, primes)
    assert err(lib.evah_keygen_switch(bare.h, RELIN, 0, D, p_e, p_s, 1, p_c0)) == "secret key not present"
    assert bare.key_bytes() == 0
    bare.close()
    g = _secret_ctx(N, primes, rng)
    # the messages key_shape and the uploads share
    for elt in (4, 2 * N + 1):
        msg = err(lib.evah_keygen_switch(g.h, GALOIS, elt, D, p_e, p_s, 1, p_c0))
        assert msg == err(lib.evah_key_upload_seeded(g.h, GALOIS, elt, D, p_c0, p_s)) == "Galois element is not valid"
    for d in (0, D + 1):
        msg = err(lib.evah_keygen_switch(g.h, RELIN, 0, d, p_e, p_s, 1, p_c0))
        assert msg == err(lib.evah_key_upload_seeded(g.h, RELIN, 0, d, p_c0, p_s)) == "invalid key digit count"
    msg = err(lib.evah_keygen_switch(g.h, 7, 0, D, p_e, p_s, 1, p_c0))
    assert msg == err(lib.evah_key_upload_seeded(g.h, 7, 0, D, p_c0, p_s)) == "unknown key kind"
    # its own
    assert "error pointer is null" in err(lib.evah_keygen_switch(g.h, RELIN, 0, D, None, p_s, 1, p_c0))
    assert "seed pointer is null" in err(lib.evah_keygen_switch(g.h, RELIN, 0, D, p_e, None, 1, p_c0))
    assert "neither installed nor returned" in err(lib.evah_keygen_switch(g.h, RELIN, 0, D, p_e, p_s, 0, None))
    # a capturing context (one real call is captured around the refusal, so that the graph is an ordinary one)
    A = g.upload_ct(np.zeros((2, D, N), dtype=np.uint64), 2.0 ** 30)
    g.capture_begin()
    try:
        B = g.negate(A)
        assert "cannot be captured" in err(lib.evah_keygen_switch(g.h, RELIN, 0, D, p_e, p_s, 1, p_c0))
    finally:
        g.graph_free(g.capture_end())
    del A, B
    assert g.key_bytes() == 0
    with pytest.raises(backend.EvaHipError, match="no such key"):
        g.key_words(RELIN, 0, 0)
    # a limb shard holds rows of the keys and no whole secret key
    g.set_shard(1, 2)
    assert err(lib.evah_keygen_switch(g.h, RELIN, 0, D, p_e, p_s, 1, p_c0)) == "a limb shard holds no whole secret key"
    assert g.key_bytes() == 0
    g.close()
