"""GPU: the refresh.  k_refresh_lift at its arithmetic edges through the C-ABI against the Python-integer
model (tests/refresh_model.py), each of its five forms at the first and last level it serves with the sign decided at every
digit position (tests/refresh_edges.py), ciphertext sizes 1 and 3, the handle forms the call reads in place, the device
against the host twin, what a refreshed value decrypts to, and a computation four times as deep as its modulus chain,
end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import refresh_model as rm
from refresh_edges import CHAINS, FORM_CASES, edge_messages, form_case_id, form_levels_out, form_messages
from eva import EvaProgram, Input, Output, load
from eva.ckks import CKKSCompiler, CKKSParameters, CKKSSignature, CKKSEncodingInfo
from eva.metric import valuation_mse
from eva.seal import generate_keys, SEALValuation
from eva_amd import backend
from eva_amd._eva import Type
from eva_amd.hostref import coeff_modulus_create

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_BITS = 20


def key(i):
    return bytes((i * 37 + j * 11 + 5) % 256 for j in range(32))


_envs = {}


def env(chain, N):
    """a device context with a secret key uploaded (uniform rows: the algebra does not need a small key) and the model's view of it"""
    if (chain, N) not in _envs:
        primes = coeff_modulus_create(N, CHAINS[chain])
        rng = np.random.default_rng(len(chain) + N)
        s = np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in primes])
        g = backend.Context(N, primes)
        g.upload_secret_key(s)
        _envs[(chain, N)] = (g, rm.Chain(N, primes, s))
    return _envs[(chain, N)]


@pytest.mark.parametrize("l_of", ["1", "2", "k-1"])
@pytest.mark.parametrize("N", [1024, 4096])
@pytest.mark.parametrize("chain", ["mixed", "all60"])
def test_kernel_edges_against_the_integer_model(chain, N, l_of):
    g, ch = env(chain, N)
    k = len(ch.primes)
    l = {"1": 1, "2": 2, "k-1": k - 1}[l_of]
    for t in (0, 1, 31, 62):
        M = edge_messages(ch.primes, l, t, N, 7 * l + t)
        ct = g.upload_ct(rm.message_ciphertext(ch, M, l), 2.0 ** (B_BITS + t))
        Mp = [rm.divide(v, t) for v in M]
        for L in sorted({1, l, k - 1}):
            ek, sd = key(3 * t + L), key(100 + 3 * t + L)
            out = g.refresh_handles([ct], L, 2.0 ** B_BITS, [ek], [sd])
            assert (out.size, out.limbs, out.scale, out.batch) == (2, L, 2.0 ** B_BITS, 1)
            want = rm.encrypt_integers(ch, Mp, L, ek, sd)
            got = out.download()
            bad = np.argwhere(got != want)
            assert bad.size == 0, (chain, N, l, L, t, "first differing (poly, limb, n)", bad[0], "M", M[bad[0][2]])


@pytest.mark.parametrize("case", FORM_CASES, ids=form_case_id)
def test_every_kernel_form_at_both_of_its_edges(case):
    """k_refresh_lift<4>, <8> and <16> at their first and last level, <62> at l = 17, 20, 32 and 61, to one prime, to the
    value's own primes and to every prime but the last, on the edge list whose sign decision falls on every digit position
    in both directions (refresh_edges.py; test_refresh_cpu.py accounts for what each list reaches).  All N coefficients of
    every limb of both polynomials are compared.  The transforms of the divided messages are formed once per t for the
    largest L: almost all of an id's time is the integer model's"""
    chain, l, ts = case
    N = 1024
    g, ch = env(chain, N)
    Ls = form_levels_out(case)
    for t in ts:
        M = form_messages(ch.primes, l, t, N)
        ct = g.upload_ct(rm.message_ciphertext(ch, M, l), 2.0 ** (B_BITS + t))
        rows = rm.transformed(ch, [rm.divide(v, t) for v in M], Ls[-1])
        ek = key(3 * t)
        for L in Ls:
            sd = key(100 + 3 * t + L)
            out = g.refresh_handles([ct], L, 2.0 ** B_BITS, [ek], [sd])
            assert (out.size, out.limbs, out.scale, out.batch) == (2, L, 2.0 ** B_BITS, 1)
            want = rm.encrypt_integers(ch, None, L, ek, sd, rows=rows)
            got = out.download()
            bad = np.argwhere(got != want)
            assert bad.size == 0, (chain, N, l, L, t, "first differing (poly, limb, n)", bad[0], "M", M[bad[0][2]])


def random_cts(ch, rng, size, limbs, n):
    """[n][size][limbs][N] uniform words: with the uniform key every product of k_decrypt_dot matters"""
    return np.stack([np.stack([np.stack([rng.integers(0, ch.primes[i], size=ch.N, dtype=np.uint64) for i in range(limbs)])
                               for _ in range(size)]) for _ in range(n)])


@pytest.mark.parametrize("l", [4, 9, 17])
@pytest.mark.parametrize("size", [1, 3])
def test_sizes_one_and_three_against_the_integer_model(size, l):
    g, ch = env("mixed21", 1024)
    k, t = len(ch.primes), 1
    words = random_cts(ch, np.random.default_rng(10 * l + size), size, l, 1)[0]
    M = rm.decrypt_integers(ch, words)
    assert max(M) > 0 > min(M)
    ct = g.upload_ct(words, 2.0 ** (B_BITS + t))
    rows = rm.transformed(ch, [rm.divide(v, t) for v in M], k - 1)
    ek = key(l)
    for L in (1, k - 1):
        sd = key(50 + L)
        out = g.refresh_handles([ct], L, 2.0 ** B_BITS, [ek], [sd])
        assert (out.size, out.limbs, out.scale, out.batch) == (2, L, 2.0 ** B_BITS, 1)
        bad = np.argwhere(out.download() != rm.encrypt_integers(ch, None, L, ek, sd, rows=rows))
        assert bad.size == 0, (size, l, L, "first differing (poly, limb, n)", bad[0], "M", M[bad[0][2]])


@pytest.mark.parametrize("l", [16, 17])
def test_64_instances_at_the_last_unrolled_level_and_the_first_looped_one(l):
    """blockIdx.y = 0 .. 63 through k_refresh_lift<16> and through <62>, whose digits live in scratch memory: every
    instance gives the words of the single call on its words, the first and the last those of the model as well"""
    g, ch = env("mixed21", 1024)
    N, k, t = 1024, len(ch.primes), 31
    L, scale = k - 1, 2.0 ** (B_BITS + t)
    rng = np.random.default_rng(l)
    single = g.upload_ct(random_cts(ch, rng, 2, l, 1)[0], scale)
    big = g.upload_ct_batch(random_cts(ch, rng, 2, l, 61), scale)
    handles = [single, big, big.unstack(60), big.unstack(7)]
    words = [single.download()] + list(big.download()) + [big.unstack(60).download(), big.unstack(7).download()]
    assert len(words) == 64
    eks, sds = [key(i) for i in range(64)], [key(200 + i) for i in range(64)]
    out = g.refresh_handles(handles, L, 2.0 ** B_BITS, eks, sds)
    assert (out.size, out.limbs, out.scale, out.batch) == (2, L, 2.0 ** B_BITS, 64)
    got = out.download().reshape(64, 2, L, N)
    for i in range(64):
        one = g.refresh_handles([g.upload_ct(words[i], scale)], L, 2.0 ** B_BITS, [eks[i]], [sds[i]]).download()
        assert np.array_equal(got[i], one), (l, i)
    for i in (0, 63):
        assert np.array_equal(got[i], rm.refresh(ch, words[i], L, t, eks[i], sds[i])), (l, i)


def _err(fn, *a):
    with pytest.raises(backend.EvaHipError) as e:
        fn(*a)
    return str(e.value)


def test_handle_forms_give_the_words_of_each_alone():
    g, ch = env("mixed", 1024)
    N, l, L, t = 1024, 3, 5, 1
    rng = np.random.default_rng(2)

    def rand_ct(limbs, n):
        return np.stack([np.stack([np.stack([rng.integers(0, ch.primes[i], size=N, dtype=np.uint64) for i in range(limbs)])
                                   for _ in range(2)]) for _ in range(n)])

    scale = 2.0 ** (B_BITS + t)
    single = g.upload_ct(rand_ct(l, 1)[0], scale)
    big = g.upload_ct_batch(rand_ct(l, 61), scale)
    switched = g.mod_switch(g.upload_ct(rand_ct(l + 1, 1)[0], scale))   # a view with the polynomial stride of l + 1 limbs
    assert switched.limbs == l

    def alone(handles):
        words = []
        for h in handles:
            w = h.download()
            words += [w] if h.batch == 1 else list(w)
        return words

    for handles in ([single], [single, big.unstack(4), big.slice(10, 6), switched], [single, big, big.unstack(60), switched]):
        words = alone(handles)
        n = len(words)
        assert n in (1, 9, 64)
        eks, sds = [key(i) for i in range(n)], [key(200 + i) for i in range(n)]
        out = g.refresh_handles(handles, L, 2.0 ** B_BITS, eks, sds)
        assert out.batch == n
        got = out.download().reshape(n, 2, L, N)
        for i in range(n):
            one = g.refresh_handles([g.upload_ct(words[i], scale)], L, 2.0 ** B_BITS, [eks[i]], [sds[i]]).download()
            assert np.array_equal(got[i], one), (n, i)
        if n == 9:   # one of them against the model as well: the view read through its own stride
            assert np.array_equal(got[8], rm.refresh(ch, words[8], L, t, eks[8], sds[8]))
    keys65 = [key(i) for i in range(65)]
    assert "more than 64 instances" in _err(g.refresh_handles, [single, big, big.unstack(0), big.unstack(1), switched], L, 2.0 ** B_BITS, keys65, keys65)
    other = g.upload_ct(rand_ct(2, 1)[0], scale)
    assert _err(g.refresh_handles, [single, other], L, 2.0 ** B_BITS, keys65[:2], keys65[:2]) == "ciphertext 1: limb count differs from ciphertext 0"
    rescaled = g.upload_ct(rand_ct(l, 1)[0], 2.0 * scale)
    assert _err(g.refresh_handles, [single, single, rescaled], L, 2.0 ** B_BITS, keys65[:3], keys65[:3]) == "ciphertext 2: scale differs from ciphertext 0"


def test_refusals_and_hygiene():
    g, ch = env("all60", 1024)
    rng = np.random.default_rng(3)
    ct = g.upload_ct(np.stack([np.stack([rng.integers(0, ch.primes[i], size=1024, dtype=np.uint64) for i in range(2)]) for _ in range(2)]), 2.0 ** 30)
    k1, k2 = [key(1)], [key(2)]
    g.sync()
    before = g.mem_info()[0]
    assert _err(g.refresh_handles, [ct], 4, 2.0 ** 30, k1, k2) == "invalid limb count for this context"
    assert _err(g.refresh_handles, [ct], 0, 2.0 ** 30, k1, k2) == "invalid limb count for this context"
    assert g.mem_info()[0] == before
    assert "target scale is above" in _err(g.refresh_handles, [ct], 3, 2.0 ** 31, k1, k2)
    assert "power of two" in _err(g.refresh_handles, [ct], 3, 3.0 * 2.0 ** 20, k1, k2)
    assert _err(g.refresh_handles, [ct], 3, 2.0 ** 30, None, k2) == "error polynomial and seed are required"
    assert _err(g.refresh_handles, [ct], 3, 2.0 ** 30, k1, None) == "error polynomial and seed are required"
    assert g.mem_info()[0] == before
    far = g.upload_ct(ct.download(), 2.0 ** 63)
    assert "exceeds 2^62" in _err(g.refresh_handles, [far], 3, 1.0, k1, k2)
    far.free()
    g.capture_begin()
    try:
        msg = _err(g.refresh_handles, [ct], 3, 2.0 ** 30, k1, k2)
    finally:
        g.graph_free(g.capture_end())
    assert "cannot be captured" in msg
    bare = backend.Context(1024, ch.primes)
    assert _err(bare.refresh_handles, [bare.upload_ct(ct.download(), 2.0 ** 30)], 3, 2.0 ** 30, k1, k2) == "secret key not present"
    # the call counts the 64 bytes of randomness per instance and brings nothing back
    up0, down0 = g.transfer_stats()[4:6]
    out = g.refresh_handles([ct], 3, 2.0 ** 30, k1, k2)
    up1, down1 = g.transfer_stats()[4:6]
    assert (up1 - up0, down1 - down0) == (64, 0) and out.limbs == 3
    g.sync()
    del out
    assert g.mem_info()[0] == before


def _step_program():
    prog = EvaProgram("step", vec_size=64)
    with prog:
        x = Input("x")
        Output("y", x * x * 0.5 + 0.25 * x)
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.poly_modulus_degree = 4096
    return compiled, params, sig


def _step(x):
    return x * x * 0.5 + 0.25 * x


_CHILD = """
import sys
sys.path.insert(0, 'tests')
import test_gpu_refresh
from eva import save
save(getattr(test_gpu_refresh, sys.argv[2])(), sys.argv[1])
"""


def twin_case():
    """two encrypted inputs refreshed for one seed: one down three levels and to scale 2^20, one up two levels at its scale"""
    params = CKKSParameters([60, 30, 45, 50, 33, 60], set(), 1024)
    pub, sec = generate_keys(params, 7)
    sig_in = CKKSSignature(64, {"a": CKKSEncodingInfo(Type.Cipher, 30, 0), "b": CKKSEncodingInfo(Type.Cipher, 30, 2)})
    xs = np.random.default_rng(4).uniform(-2, 2, (2, 64))
    enc = sec.encrypt({"a": xs[0].tolist(), "b": xs[1].tolist()}, sig_in, seed=3)
    sig_out = CKKSSignature(64, {"a": CKKSEncodingInfo(Type.Cipher, 20, 3), "b": CKKSEncodingInfo(Type.Cipher, 30, 0)})
    return sec.refresh(enc, sig_out, seed=5)


def twin_case_long():
    """the same on 19 primes of 60 bits: one value down from 17 limbs to 3 and to scale 2^20 (k_refresh_lift<62>), one up
    from 2 limbs to 17"""
    params = CKKSParameters([60] * 19, set(), 1024)
    pub, sec = generate_keys(params, 7)
    sig_in = CKKSSignature(64, {"a": CKKSEncodingInfo(Type.Cipher, 30, 1), "b": CKKSEncodingInfo(Type.Cipher, 30, 16)})
    xs = np.random.default_rng(4).uniform(-2, 2, (2, 64))
    enc = sec.encrypt({"a": xs[0].tolist(), "b": xs[1].tolist()}, sig_in, seed=3)
    assert (enc.get("a")[2], enc.get("b")[2]) == (17, 2)
    sig_out = CKKSSignature(64, {"a": CKKSEncodingInfo(Type.Cipher, 20, 15), "b": CKKSEncodingInfo(Type.Cipher, 30, 1)})
    return sec.refresh(enc, sig_out, seed=5)


def _device_equals_host_twin(tmp_path, case, limbs):
    path = str(tmp_path / "host.sealvals")
    child_env = dict(os.environ, PYTHONPATH=ROOT, EVA_DEVICE_CLIENT="0")
    out = subprocess.run([sys.executable, "-c", _CHILD, path, case], cwd=ROOT, env=child_env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    host, dev = load(path), globals()[case]()
    assert dev.is_resident("a")
    for name in ("a", "b"):
        h, d = host.get(name), dev.get(name)
        assert h[:4] == d[:4] and np.array_equal(h[4], d[4]), name
        assert host.seed(name) == dev.seed(name)
    assert (dev.get("a")[2], dev.get("b")[2]) == limbs


def test_device_equals_host_twin(tmp_path):
    _device_equals_host_twin(tmp_path, "twin_case", (2, 5))   # "a" went down three levels, "b" up two


def test_device_equals_host_twin_on_19_primes(tmp_path):
    _device_equals_host_twin(tmp_path, "twin_case_long", (3, 17))


def test_a_refreshed_value_decrypts_to_the_original():
    """each coefficient moves by at most 21 (sample_error's bound) + 1/2 (the rounding); a slot is a sum of N coefficients
    with weights of modulus 1 over the scale 2^b: 22 N / 2^b leaves 1/2 per coefficient for the FP64 decode"""
    N = 1024
    pub, sec = generate_keys(CKKSParameters([60, 30, 45, 50, 33, 60], set(), N), 7)
    sig_in = CKKSSignature(64, {"x": CKKSEncodingInfo(Type.Cipher, 30, 1)})
    xs = np.random.default_rng(5).uniform(-2, 2, 64)
    enc = sec.encrypt({"x": xs.tolist()}, sig_in, seed=3)
    ref = np.array(sec.decrypt(enc, sig_in)["x"])
    for b, level in ((30, 0), (20, 0), (20, 3), (12, 4)):
        sig = CKKSSignature(64, {"x": CKKSEncodingInfo(Type.Cipher, b, level)})
        got = np.array(sec.decrypt(sec.refresh(enc, sig, seed=9), sig)["x"])
        diff = float(np.abs(got - ref).max())
        print(f"refresh to scale 2^{b}, level {level}: max slot difference {diff:.3e}, bound {22 * N / 2.0 ** b:.3e}")
        assert diff <= 22 * N / 2.0 ** b, (b, level, diff)


def test_four_passes_on_a_chain_that_allows_one():
    compiled, params, sig = _step_program()
    pub, sec = generate_keys(params, 3)
    xs = np.random.default_rng(0).uniform(-1, 1, 64)
    enc = sec.encrypt({"x": xs.tolist()}, sig, seed=1)
    want = xs
    for p in range(4):
        out = pub.execute(compiled, enc)
        want = _step(want)
        if p == 3:
            break
        pub.synchronize()
        before = pub.transfer_stats()
        enc = sec.refresh(out, sig, rename={"x": "y"}, seed=10 + p)
        after = pub.transfer_stats()
        assert after["h2d_bytes"] - before["h2d_bytes"] == 64 and after["d2h_bytes"] == before["d2h_bytes"]
        assert after["ct_downloads"] == before["ct_downloads"] and enc.is_resident("x") and enc.seed("x") is not None
    mse = valuation_mse(sec.decrypt(out, sig), {"y": want.tolist()})
    print(f"four passes, three refreshes, N = 4096, chain {list(params.prime_bits)}: mse {mse:.3e}")
    assert mse < 0.01
    # the chain really was exhausted: the unrefreshed output is no input of the next pass
    kind, size, limbs, scale, words = out.get("y")
    stale = SEALValuation()
    stale._set_cipher("x", words, scale)
    with pytest.raises(Exception):
        pub.execute(compiled, stale)
        pub.synchronize()


def test_four_passes_of_a_batch_of_70():
    compiled, params, sig = _step_program()
    pub, sec = generate_keys(params, 3)
    xs = np.random.default_rng(1).uniform(-1, 1, (70, 64))
    vb = sec.encrypt_array({"x": xs}, sig, seed=2)
    want = xs
    for p in range(4):
        outs = pub.execute_batch(compiled, vb)
        want = _step(want)
        if p == 3:
            break
        pub.synchronize()
        before = pub.transfer_stats()
        vb = sec.refresh(outs, sig, rename={"x": "y"}, seed=20 + p)
        after = pub.transfer_stats()
        assert after["h2d_bytes"] - before["h2d_bytes"] == 64 * 70 and after["d2h_bytes"] == before["d2h_bytes"]
        assert len(vb) == 70 and vb.segments("x") == [64, 6]   # two calls; the results go back in as batched handles
    got = sec.decrypt_array(outs, sig)["y"]
    mse = float(np.mean((got - want) ** 2))
    print(f"batch of 70, four passes, three refreshes: mse {mse:.3e}")
    assert mse < 0.01
    assert valuation_mse({"y": got[69].tolist()}, {"y": want[69].tolist()}) < 0.01
    # a seeded batch refreshes to the words of the list path's instance, for one seed
    again = sec.refresh(outs, sig, rename={"x": "y"}, seed=77)
    single = sec.refresh(outs[0], sig, rename={"x": "y"}, seed=77)
    assert np.array_equal(again[0].get("x")[4], single.get("x")[4]) and again[0].seed("x") == single.seed("x")
