"""GPU: re-key to another key pair at the C-ABI — evah_keygen_rekey, the key kind EVAH_KEY_REKEY and
evah_rekey_many.

Key generation.  For N in {1024 (below one SAMPLE_TILE: the partial-tile branch of k_sample_small), 4096 (the wide tile)}
and the chains [60, 30, 45, 50, 33, 60] and [60] * 4, with k - 1 digits: the device's key equals the host twin
(rekey_keygen_host) and the Python-integer model word for word, and decrypts digit by digit per the key equation:
c0 + c1 sB - [i == J] P sA has centred coefficients of at most 21 (2 N + 1).

Application.  evah_rekey_many equals oracle.switch_key((c0, 0), c1, key) bit for bit, per context at l in {1, 2, k - 1}
(the lower levels are mod-switched views of the top-level uploads), for n in {1, 3, 64} single handles, 65 instances
across the chunk boundary (a batched handle of 64 — the most a handle holds — and a single one; 70 through two slices,
the boundary inside the second), through an evah_ct_slice and an evah_ct_unstack view, and for handles owned
by a second context of the same GPU, read in place.  Inputs: random residues, every c1 residue q_i - 1, and — under
[60] * 4, the chain they were searched for — the bound-reaching words of tests/lazy_bound_words.py for that N as c1
(tests/golden/lazy_bound_words_N4096.npy is `python tests/lazy_bound_words.py 12`: late values 1.002 .. 1.013 x 2^64).  Contexts, as
tests/test_gpu_single_is_batch.py chooses its own:
  N1024_mixed  [60, 30, 45, 50, 33, 60]            partial tile, two-launch form; primes below 2^54 beside top-bit primes
  N1024_60x4   [60] * 4                            the stored worst-case words at the partial tile
  small        N = 4096, [60] * 4                  small-launch form, MAC3
  modup        the same, EVAH_FUSE_SMALL=0         mod-up kernel with MAC3
  N4096_mixed  N = 4096, the mixed chain           no MAC3 at the wide tile
  fold_pa0     N = 4096, [60] * 4, EVAH_FOLD_PA=0  c0 joins in the mod-down's combine pass (add_tab)
The references of a context are computed once and shared by its tests."""
import numpy as np
import pytest

import rekey_model as rm
from eva_amd import backend
from lazy_bound_words import bound_reaching_poly
from oracle import pyoracle as po
from test_gpu_extremes import _ctx, _same

pytestmark = pytest.mark.gpu

SLOT = 7
CONTEXTS = [
    ("N1024_mixed", 1 << 10, rm.CHAINS["mixed"], {}),
    ("N1024_60x4", 1 << 10, rm.CHAINS["60x4"], {}),
    ("small", 1 << 12, rm.CHAINS["60x4"], {}),
    ("modup", 1 << 12, rm.CHAINS["60x4"], {"EVAH_FUSE_SMALL": 0}),
    ("N4096_mixed", 1 << 12, rm.CHAINS["mixed"], {}),
    ("fold_pa0", 1 << 12, rm.CHAINS["60x4"], {"EVAH_FOLD_PA": 0}),
]
N_INST = 65


def _rand(rng, primes, N, prefix, nl):
    return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))


class _Case:
    """one context holding a random re-key key, 65 random size-2 ciphertexts at the top level and, per level, what the
    oracle makes of them"""

    def __init__(self, name, N, bits, knobs):
        self.name, self.N, self.bits, self.primes = name, N, bits, po.coeff_modulus_create(N, bits)
        self.k = len(self.primes)
        self.top = self.k - 1
        self.levels = sorted({1, 2, self.top})
        self.o = po.Oracle(N, self.primes)
        self.rng = np.random.default_rng(N + len(bits) + 7 * len(knobs))
        self.key = _rand(self.rng, self.primes, N, (self.top, 2), self.k)
        self.g = _ctx(N, self.primes, knobs)
        self.g.upload_rekey_key(SLOT, self.key)
        self.cts = _rand(self.rng, self.primes, N, (N_INST, 2), self.top)
        self._ref = {}

    def want(self, l, b):
        """the re-key of instance b at level l (the first l limbs of the upload)"""
        if (l, b) not in self._ref:
            self._ref[l, b] = self.rekey(np.ascontiguousarray(self.cts[b][:, :l]))
        return self._ref[l, b]

    def rekey(self, ct):
        ct2 = ct.copy()
        ct2[1] = 0
        return self.o.switch_key(ct2, np.ascontiguousarray(ct[1]), self.key)

    def at_level(self, h, l):
        for _ in range(self.top - l):
            h = self.g.mod_switch(h)
        return h


@pytest.fixture(scope="module", params=CONTEXTS, ids=[c[0] for c in CONTEXTS])
def case(request):
    p = _Case(*request.param)
    yield p
    p.g.close()


def test_single_handles_at_every_level(case):
    p, g = case, case.g
    ups = [g.upload_ct(p.cts[b], 2.0 ** 40) for b in range(64)]
    for l in p.levels:
        hs = [p.at_level(h, l) for h in ups]  # l < top: mod-switched views, polynomial stride of the top level
        for n in (1, 3, 64):
            outs = g.rekey_many(SLOT, hs[:n])
            assert len(outs) == n
            for b in range(n):
                assert outs[b].info() == (2, l, 2.0 ** 40) and outs[b].batch == 1
                _same(outs[b].download(), p.want(l, b), f"{p.name} l={l} n={n} instance {b}")
    direct = g.upload_ct(np.ascontiguousarray(p.cts[0][:, :1]), 2.0 ** 40)  # the same level-1 value as an upload of its own
    _same(g.rekey_many(SLOT, [direct])[0].download(), p.want(1, 0), "uploaded at level 1")


def test_65_instances_across_the_chunk_boundary_slices_and_views(case):
    """a batched handle holds at most 64 instances (evah_ct_upload_batch refuses more), so the 65 instances that cross the
    chunk boundary are a batched handle of 64 and a single one; then 70 through two overlapping slices, where the boundary
    falls inside the second handle"""
    p, g = case, case.g
    B = g.upload_ct_batch(p.cts[:64], 2.0 ** 30)
    last = g.upload_ct(p.cts[64], 2.0 ** 30)
    for l in p.levels:
        outs = g.rekey_many(SLOT, [p.at_level(B, l), p.at_level(last, l)])
        assert [o.batch for o in outs] == [64, 1] and all(o.info() == (2, l, 2.0 ** 30) for o in outs)
        got = outs[0].download()
        for b in range(64):
            _same(got[b], p.want(l, b), f"{p.name} l={l} batched instance {b}")
        _same(outs[1].download(), p.want(l, 64), f"{p.name} l={l} instance 64, the second chunk")
    l = p.levels[-1]
    outs = g.rekey_many(SLOT, [B.slice(0, 40), B.slice(20, 30)])  # 70 instances: the second handle spans both chunks
    assert [o.batch for o in outs] == [40, 30]
    for out, b0 in zip(outs, (0, 20)):
        got = out.download()
        for j in range(out.batch):
            _same(got[j], p.want(l, b0 + j), f"slice from {b0}, instance {j}")
    sl, un, single = B.slice(59, 5), B.unstack(63), g.upload_ct(p.cts[2], 2.0 ** 30)
    outs = g.rekey_many(SLOT, [sl, un, single])  # handles of 5, 1 and 1 instances in one call
    assert [o.batch for o in outs] == [5, 1, 1]
    got = outs[0].download()
    for j in range(5):
        _same(got[j], p.want(l, 59 + j), f"slice instance {j}")
    _same(outs[1].download(), p.want(l, 63), "unstacked view")
    _same(outs[2].download(), p.want(l, 2), "single handle beside views")


def test_handles_of_another_context_are_read_in_place(case):
    p, g = case, case.g
    other = backend.Context(p.N, p.primes)  # the device state of another key pair on the same GPU
    try:
        before = g.transfer_stats()
        hs = [other.upload_ct(p.cts[b], 2.0 ** 40) for b in range(3)]
        hb = other.upload_ct_batch(p.cts[3:6], 2.0 ** 40)
        prod = other.add(hs[0], hs[1])  # not synchronised with the host: ordered behind its producer by acquire()
        outs = g.rekey_many(SLOT, hs + [hb, prod])
        assert g.transfer_stats() == before, "no ciphertext crossed the host boundary on the destination"
        for b in range(3):
            _same(outs[b].download(), p.want(p.top, b), f"foreign handle {b}")
        got = outs[3].download()
        for j in range(3):
            _same(got[j], p.want(p.top, 3 + j), f"foreign batched instance {j}")
        _same(outs[4].download(), p.rekey(p.o.add(p.cts[0], p.cts[1])), "foreign result in flight")
        del outs, hs, hb, prod
    finally:
        other.close()


def test_worst_case_words(case):
    p, g = case, case.g
    worst = _rand(p.rng, p.primes, p.N, (2,), p.top)
    for i in range(p.top):
        worst[1, i, :] = p.primes[i] - 1
    inputs = [("every c1 residue q_i - 1", worst)]
    if p.bits == rm.CHAINS["60x4"]:  # the stored inputs belong to coeff_modulus_create(N, [60] * 4): digit 0 under prime 1
        coeff = bound_reaching_poly(p.N)
        lazy = _rand(p.rng, p.primes, p.N, (2,), p.top)
        lazy[1] = np.stack([p.o.ntt(i, coeff % np.uint64(p.primes[i])) for i in range(p.top)])
        inputs.append(("bound-reaching words", lazy))
    for what, ct in inputs:
        for l in p.levels:
            h = p.at_level(g.upload_ct(ct, 2.0 ** 40), l)
            _same(g.rekey_many(SLOT, [h])[0].download(), p.rekey(np.ascontiguousarray(ct[:, :l])), f"{p.name} {what} l={l}")
        hb = g.upload_ct_batch(np.stack([ct] * 3), 2.0 ** 40)
        got = g.rekey_many(SLOT, [hb])[0].download()
        for b in range(3):
            _same(got[b], p.rekey(ct), f"{p.name} {what}, batched instance {b}")


def test_split_copy_follows_the_other_kinds(case):
    p, g = case, case.g
    words = g.key_words(backend.KEY_REKEY, SLOT)
    _same(words, p.key, "installed key words")
    g.upload_relin_key(p.key)
    try:
        g.key_words(backend.KEY_RELIN, 0, which=1)
        relin_split = True
    except backend.EvaHipError:
        relin_split = False
    if relin_split:
        _same(g.key_words(backend.KEY_REKEY, SLOT, which=1), g.key_words(backend.KEY_RELIN, 0, which=1), "split copy")
    else:
        with pytest.raises(backend.EvaHipError, match="no split copy"):
            g.key_words(backend.KEY_REKEY, SLOT, which=1)
    print(p.name, "split copy:", relin_split)


# ---- key generation
KEYGEN = [(N, chain) for N in (1 << 10, 1 << 12) for chain in ("mixed", "60x4")]


@pytest.mark.parametrize("N,chain", KEYGEN, ids=[f"N{N}_{c}" for N, c in KEYGEN])
def test_keygen_equals_the_host_twin_and_the_key_equation(N, chain):
    from eva_amd import _eva
    primes = po.coeff_modulus_create(N, rm.CHAINS[chain])
    o = po.Oracle(N, primes)
    rng = np.random.default_rng(N + len(primes))
    A, B = rm.KeyPair(o, rng), rm.KeyPair(o, rng)
    D = len(primes) - 1
    rkeys = np.frombuffer(rng.bytes(32 * D), dtype=np.uint8).reshape(D, 32)
    g = backend.Context(N, primes)
    try:
        g.upload_secret_key(A.s_ntt)
        own_pk = _rand(rng, primes, N, (2,), len(primes))
        g.upload_public_key(own_pk)
        before = g.transfer_stats()
        key = g.keygen_rekey(B.pk, rkeys)
        after = g.transfer_stats()
        assert after[4] - before[4] == B.pk.nbytes + 32 * D and after[5] - before[5] == key.nbytes
        twin = _eva._seal._rekey_keygen_host(N, primes, A.s_ntt, B.pk, rkeys)
        _same(key.reshape(D * 2, len(primes), N), twin.reshape(D * 2, len(primes), N), "device against the host twin")
        if N == 1 << 10:  # the integer model once per chain (tests/test_rekey_cpu.py holds the twin to it at this size)
            _same(key.reshape(D * 2, len(primes), N), rm.model_key(o, B.pk, A.s_ntt, rkeys).reshape(D * 2, len(primes), N), "model")
        noise = rm.key_noise(o, key, A.s_ntt, B.s_ntt)
        print(f"N={N} {chain}: key noise {noise}, bound {rm.noise_bound(N)}")
        assert 0 < noise <= rm.noise_bound(N)
        # the context's own public key is still the one it had: an encryption of zero under it has not changed
        fewer = g.keygen_rekey(B.pk, rkeys[:2])  # fewer digits: the same leading digits
        _same(fewer.reshape(4, len(primes), N), key[:2].reshape(4, len(primes), N), "two digits")
    finally:
        g.close()


# ---- refusals
def test_refusals_with_their_messages():
    N = 1 << 10
    primes = po.coeff_modulus_create(N, [60, 60, 60])
    k, rng = len(primes), np.random.default_rng(3)
    g = backend.Context(N, primes)
    try:
        key = _rand(rng, primes, N, (k - 1, 2), k)
        a2 = g.upload_ct(_rand(rng, primes, N, (2,), k - 1), 2.0 ** 30)
        a3 = g.upload_ct(_rand(rng, primes, N, (3,), k - 1), 2.0 ** 30)
        with pytest.raises(backend.EvaHipError, match="re-key key not present"):
            g.rekey_many(SLOT, [a2])
        g.upload_rekey_key(SLOT, key)
        with pytest.raises(backend.EvaHipError, match="re-key key not present"):
            g.rekey_many(SLOT + 1, [a2])
        with pytest.raises(backend.EvaHipError, match=r"re-key expects a size-2 ciphertext \(relinearize first\)"):
            g.rekey_many(SLOT, [a3])
        with pytest.raises(backend.EvaHipError, match="encrypted parameter mismatch in batch"):
            g.rekey_many(SLOT, [a2, g.mod_switch(a2)])
        seeds = np.zeros((k - 1, 32), dtype=np.uint8)
        with pytest.raises(backend.EvaHipError, match="not seed-compressible"):
            g._upload_key_seeded(backend.KEY_REKEY, SLOT, key[:, 0], seeds)
        g.upload_secret_key(_rand(rng, primes, N, (), k))
        with pytest.raises(backend.EvaHipError, match="generated by evah_keygen_rekey"):
            g.keygen_switch(backend.KEY_REKEY, SLOT, np.zeros((k - 1, N), dtype=np.int8), seeds)
        with pytest.raises(backend.EvaHipError, match="generated by evah_keygen_rekey"):
            g.keygen_set([(backend.KEY_REKEY, SLOT)], seeds[None], seeds[None])
        pk = _rand(rng, primes, N, (2,), k)
        with pytest.raises(backend.EvaHipError, match="invalid key digit count"):
            g.keygen_rekey(pk, np.zeros((k, 32), dtype=np.uint8))
        g.capture_begin()
        try:
            neg = g.negate(a2)  # (an empty capture is no graph)
            with pytest.raises(backend.EvaHipError, match="cannot be captured into a graph"):
                g.keygen_rekey(pk, seeds)
            with pytest.raises(backend.EvaHipError, match="cannot be captured into a graph"):
                g.rekey_many(SLOT, [a2])
        finally:
            g.graph_free(g.capture_end())
        del neg
        bare = backend.Context(N, primes)
        try:
            with pytest.raises(backend.EvaHipError, match="secret key not present"):
                bare.keygen_rekey(pk, seeds)
            bare.set_shard(0, 2)
            with pytest.raises(backend.EvaHipError, match="limb shard"):
                bare.keygen_rekey(pk, seeds)
            with pytest.raises(backend.EvaHipError, match="limb shard"):
                bare.rekey_many(SLOT, [a2])
        finally:
            bare.close()
    finally:
        g.close()


# ---- the public interface, end to end
import os
import subprocess
import sys

from eva import EvaProgram, Input, Output, load
from eva.ckks import CKKSCompiler, CKKSParameters
from eva.metric import valuation_mse
from eva.seal import RekeyKey, generate_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E_N, E2E_BITS, IN_SCALE = 1 << 12, [60] * 4, 50


def _square_program():
    """one multiply at input scale 2^50: no rescale follows (2^100 stays below the waterline rule), so the chain is free"""
    prog = EvaProgram("square", vec_size=64)
    with prog:
        x = Input("x")
        Output("y", x * x)
    prog.set_input_scales(IN_SCALE)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.prime_bits = list(E2E_BITS)
    params.poly_modulus_degree = E2E_N
    return compiled, params, sig


def _issue_bound(l):
    """the worst case of the key-switch sum plus the mod-down's rounding, carried to slots, over the inputs' scale 2^50
    (the value itself lives at 2^100, where the same sum is below what FP64 decoding resolves)"""
    primes = po.coeff_modulus_create(E2E_N, E2E_BITS)
    return rm.slot_bound(E2E_N, primes, l, IN_SCALE)


@pytest.fixture(scope="module")
def two_pairs():
    compiled, params, sig = _square_program()
    (pub_a, sec_a), (pub_b, sec_b) = generate_keys(params, 21), generate_keys(params, 22)
    rk = sec_a.make_rekey_key(pub_b, seed=4)
    return compiled, sig, pub_a, sec_a, pub_b, sec_b, rk


def test_end_to_end_single(two_pairs):
    compiled, sig, pub_a, sec_a, pub_b, sec_b, rk = two_pairs
    xs = np.random.default_rng(0).uniform(-1, 1, 64)
    out_a = pub_a.execute(compiled, pub_a.encrypt({"x": xs.tolist()}, sig))
    kind, size, limbs, scale, _ = out_a.get("y")
    assert (size, limbs, scale) == (2, len(E2E_BITS) - 1, 2.0 ** (2 * IN_SCALE))
    ref = np.array(sec_a.decrypt(out_a, sig)["y"])
    assert float(np.abs(np.array(sec_a.decrypt(out_a, sig)["y"]) - ref).max()) == 0.0  # the reference against itself
    assert pub_b.install_rekey_key(rk) == pub_b.install_rekey_key(rk)
    pub_a.synchronize()
    before = pub_a.transfer_stats(), pub_b.transfer_stats()
    out_b = pub_b.rekey(out_a, rk)
    assert (pub_a.transfer_stats(), pub_b.transfer_stats()) == before, "no byte crossed PCIe"
    assert out_b.is_resident("y") and out_b.get("y")[1:4] == (2, limbs, scale)
    got = np.array(sec_b.decrypt(out_b, sig)["y"])
    diff, bound = float(np.abs(got - ref).max()), _issue_bound(limbs)
    print(f"re-key A -> B, N = {E2E_N}, {E2E_BITS}, l = {limbs}: largest slot difference {diff:.3e}, bound {bound:.3e}; "
          f"against x^2 {float(np.abs(got - xs * xs).max()):.3e}")
    assert bound < 0.01 and diff <= bound
    assert float(np.abs(np.array(sec_a.decrypt(out_b, sig)["y"]) - ref).max()) > 1.0, "A no longer decrypts it"
    # a value on the host is uploaded first, and gives the same words
    kind, size, limbs, scale, words = out_a.get("y")
    from eva.seal import SEALValuation
    host = SEALValuation()
    host._set_cipher("y", words, scale)
    host._set_raw("note", [1.0, 2.0])
    again = pub_b.rekey(host, rk)
    assert np.array_equal(again.get("y")[4], out_b.get("y")[4]) and again.get("note")[-1] == [1.0, 2.0]


def test_end_to_end_batch_of_70(two_pairs):
    compiled, sig, pub_a, sec_a, pub_b, sec_b, rk = two_pairs
    xs = np.random.default_rng(1).uniform(-1, 1, (70, 64))
    outs_a = pub_a.execute_batch(compiled, pub_a.encrypt_array({"x": xs}, sig, seed=2))
    ref = sec_a.decrypt_array(outs_a, sig)["y"]
    pub_b.install_rekey_key(rk)
    pub_a.synchronize()
    before = pub_a.transfer_stats(), pub_b.transfer_stats()
    outs_b = pub_b.rekey(outs_a, rk)
    assert (pub_a.transfer_stats(), pub_b.transfer_stats()) == before, "no ciphertext byte up or down"
    assert len(outs_b) == 70 and outs_b.segments("y") == outs_a.segments("y") and sum(outs_b.segments("y")) == 70
    assert len(outs_b.segments("y")) >= 2
    got = sec_b.decrypt_array(outs_b, sig)["y"]  # accepted: the batch lives on B's device state
    diff, bound = float(np.abs(got - ref).max()), _issue_bound(len(E2E_BITS) - 1)
    print(f"batch of 70: largest slot difference {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound
    single = pub_b.rekey(outs_a[69], rk)  # the list path's instance: the same words
    assert np.array_equal(single.get("y")[4], outs_b[69].get("y")[4])
    with pytest.raises(Exception, match="another key pair"):
        sec_a.refresh(outs_b, sig, rename={"x": "y"})


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


def test_composition_rekey_refresh_execute():
    compiled, params, sig = _step_program()
    (pub_a, sec_a), (pub_b, sec_b) = generate_keys(params, 31), generate_keys(params, 32)
    rk = sec_a.make_rekey_key(pub_b)
    xs = np.random.default_rng(3).uniform(-1, 1, 64)
    step = lambda x: x * x * 0.5 + 0.25 * x
    out_a = pub_a.execute(compiled, sec_a.encrypt({"x": xs.tolist()}, sig, seed=1))
    handed = pub_b.rekey(out_a, rk)
    enc_b = sec_b.refresh(handed, sig, rename={"x": "y"}, seed=2)
    out_b = pub_b.execute(compiled, enc_b)
    mse = valuation_mse(sec_b.decrypt(out_b, sig), {"y": step(step(xs)).tolist()})
    print(f"program under A -> rekey -> refresh under B -> program under B: mse {mse:.3e}")
    assert mse < 0.01
    assert valuation_mse(sec_b.decrypt(handed, sig), {"y": step(xs).tolist()}) < 0.01


_CHILD = """
import sys
sys.path.insert(0, 'tests')
from test_gpu_rekey import twin_key
from eva import save
save(twin_key(), sys.argv[1])
"""


def twin_key():
    params = CKKSParameters([60, 30, 45, 50, 33, 60], set(), 1024)
    (_, sec_a), (pub_b, _) = generate_keys(params, 11), generate_keys(params, 12)
    before = sec_a.transfer_stats()
    rk = sec_a.make_rekey_key(pub_b, seed=5)
    twin_key.d2h = sec_a.transfer_stats()["d2h_bytes"] - before["d2h_bytes"]
    return rk


def test_make_rekey_key_device_equals_host_twin_child(tmp_path):
    path = str(tmp_path / "host.rekey")
    child_env = dict(os.environ, PYTHONPATH=ROOT, EVA_DEVICE_CLIENT="0")
    out = subprocess.run([sys.executable, "-c", _CHILD, path], cwd=ROOT, env=child_env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    host, dev = load(path), twin_key()
    assert isinstance(host, RekeyKey) and twin_key.d2h == dev.words().nbytes, "the device made the key"
    assert (host.n_digits, host.poly_modulus_degree, list(host.primes)) == (dev.n_digits, dev.poly_modulus_degree, list(dev.primes))
    _same(dev.words().reshape(-1, 6, 1024), host.words().reshape(-1, 6, 1024), "device against the host twin")
