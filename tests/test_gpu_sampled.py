"""GPU: encryption randomness drawn on the device from a 32-byte randomness key per value.
evah_encode_encrypt_sampled_many / _symmetric_sampled_many against evah_encode_encrypt_many / _symmetric_many fed the host
twin's polynomials, word for word — which ties the new kernel to the single calls and the oracle through
test_gpu_client_batch.py; the refusals of the existing calls; and encrypt_batch(..., device_sampling=True) against the
host path of the same seed, through execute_batch and decrypt_batch, with the bytes the option keeps off PCIe.
Shapes: N = 1024 is half a workgroup of the sampling kernel (128 ChaCha blocks), N = 4096 two workgroups per polynomial
and the two-pass FFT; batch 8 / 9 are the two ways seeds travel, 64 the largest call; the N = 1024 chain mixes 30-, 40-
and 41-bit primes, the N = 4096 chain 20- and 60-bit ones."""
import numpy as np
import pytest

from eva import evaluate, load, save
from eva.seal import generate_keys
from eva_amd import _eva, backend
from evatest import oracle_execute
from test_gpu_client import _flow
from test_gpu_client_batch import CHAINS, SCALE, _env_of, _err, _same

pytestmark = pytest.mark.gpu

sampled_small = _eva._seal._sampled_small


@pytest.fixture(params=[CHAINS[0], CHAINS[2]], ids=lambda c: f"N{c[0]}")
def env(request):
    return _env_of(request.param)


def _keys(env, batch):
    return [env.rng.integers(0, 256, size=32, dtype=np.uint8).tobytes() for _ in range(batch)]


def _twin(keys, N, polys):
    return np.array([[sampled_small(k, p, N) for p in polys] for k in keys], dtype=np.int8).reshape(len(keys), len(polys), N)


# ---- 1. the C-ABI calls against the existing calls on the host twin's polynomials

@pytest.mark.parametrize("batch", [1, 8, 9, 64])
def test_encode_encrypt_sampled_many_equals_the_call_on_the_twins_polynomials(env, batch):
    g, N, k = env.g, env.N, env.k
    for l in sorted({1, k - 1}):
        values = env.rng.uniform(-4, 4, (batch, 8))
        rkeys = _keys(env, batch)
        if batch > 1:
            rkeys[-1] = bytes(32)   # the all-zero key too
        ct = g.encode_encrypt_sampled_many(values, l, SCALE, rkeys)
        assert ct.batch == batch and ct.info() == (2, l, SCALE)
        want = g.encode_encrypt_many(values, l, SCALE, _twin(rkeys, N, (0, 1, 2)))
        assert np.array_equal(ct.download(), want.download()), f"l={l}"
        assert np.array_equal(ct.unstack(batch - 1).download(), want.unstack(batch - 1).download())


@pytest.mark.parametrize("batch", [1, 8, 9, 64])
def test_encode_encrypt_symmetric_sampled_many_equals_the_call_on_the_twins_error(env, batch):
    g, N, k = env.g, env.N, env.k
    for l in sorted({1, k - 1}):
        values = env.rng.uniform(-4, 4, (batch, 8))
        ekeys, seeds = _keys(env, batch), _keys(env, batch)
        ct = g.encode_encrypt_symmetric_sampled_many(values, l, SCALE, ekeys, seeds)
        assert ct.batch == batch and ct.info() == (2, l, SCALE)
        want = g.encode_encrypt_symmetric_many(values, l, SCALE, _twin(ekeys, N, (1,))[:, 0], seeds)
        assert np.array_equal(ct.download(), want.download()), f"l={l}"


def test_refusals_mirror_the_existing_calls(env):
    g, N, k = env.g, env.N, env.k
    l = k - 1
    vals = lambda b: env.rng.uniform(-1, 1, (b, 8))
    pub = lambda b: (vals(b), l, SCALE, [bytes(32)] * b)
    sym = lambda b: (vals(b), l, SCALE, [bytes(32)] * b, [bytes(32)] * b)
    for b in (0, 65):
        assert "batch must be 1..64" in _err(g.encode_encrypt_sampled_many, *pub(b))
        assert "batch must be 1..64" in _err(g.encode_encrypt_symmetric_sampled_many, *sym(b))
    # value count and limb count: the existing calls' messages
    v = vals(2)
    small, keys = env.small(2), [bytes(32)] * 2
    assert _err(g.encode_encrypt_sampled_many, v[:, :3], l, SCALE, keys) == _err(g.encode_encrypt_many, v[:, :3], l, SCALE, small)
    for limbs in (0, k):
        assert _err(g.encode_encrypt_sampled_many, v, limbs, SCALE, keys) == _err(g.encode_encrypt_many, v, limbs, SCALE, small)
        assert (_err(g.encode_encrypt_symmetric_sampled_many, v, limbs, SCALE, keys, keys)
                == _err(g.encode_encrypt_symmetric_many, v, limbs, SCALE, small[:, 0], keys))
    # null keys: the null-pointer messages of the existing calls
    assert _err(g.encode_encrypt_sampled_many, v, l, SCALE, None) == "randomness pointer is null"
    assert _err(g.encode_encrypt_symmetric_sampled_many, v, l, SCALE, None, keys) == "error polynomial and seed are required"
    assert _err(g.encode_encrypt_symmetric_sampled_many, v, l, SCALE, keys, None) == "error polynomial and seed are required"
    # a capturing context (one real call is captured around the refusals, so that the graph is an ordinary one)
    ct = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), SCALE)
    g.capture_begin()
    try:
        neg = g.negate(ct)
        cap = [_err(g.encode_encrypt_sampled_many, *pub(2)), _err(g.encode_encrypt_symmetric_sampled_many, *sym(2))]
        existing = _err(g.encode_encrypt_many, v, l, SCALE, small)
    finally:
        g.graph_free(g.capture_end())
    del neg
    assert cap == [existing] * 2 and "cannot be captured" in existing
    # missing keys
    bare = backend.Context(N, env.primes)
    try:
        assert _err(bare.encode_encrypt_sampled_many, *pub(2)) == "public key not present"
        assert _err(bare.encode_encrypt_symmetric_sampled_many, *sym(2)) == "secret key not present"
    finally:
        bare.close()


# ---- 2. through Python

def _inputs(n, vec, seed):
    rng = np.random.default_rng(seed)
    return [{'x': list(rng.uniform(-2, 2, vec)), 'y': list(rng.uniform(-2, 2, vec))} for _ in range(n)]


def test_seventy_instances_equal_the_host_path_of_the_same_seed(monkeypatch):
    compiled, params, sig = _flow(8, 1024, 30)
    xs = _inputs(70, 8, 8)
    pub, sec = generate_keys(params, 6)
    dev_pub = pub.encrypt_batch(xs, sig, device_sampling=True, seed=3)
    dev_sec = sec.encrypt_batch(xs, sig, seed=3, device_sampling=True)
    assert len(dev_pub) == len(dev_sec) == 70
    assert all(e.is_resident(n) for e in dev_pub + dev_sec for n in ('x', 'y'))
    seeds = [e.seed(n) for e in dev_sec for n in ('x', 'y')]
    assert None not in seeds and len(set(seeds)) == 140
    assert seeds == [e.seed(n) for e in sec.encrypt_batch(xs, sig, seed=3) for n in ('x', 'y')]   # c1 as without the option
    got = sec.decrypt_batch(dev_pub, sig)
    for b in range(70):
        for n in ('x', 'y'):
            assert np.abs(np.array(got[b][n]) - np.array(xs[b][n])).max() < 1e-4, (b, n)
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    pub0, sec0 = generate_keys(params, 6)   # same seed: same keys
    host_pub = pub0.encrypt_batch(xs, sig, device_sampling=True, seed=3)
    host_sec = sec0.encrypt_batch(xs, sig, seed=3, device_sampling=True)
    assert not any(e.is_resident(n) for e in host_pub + host_sec for n in ('x', 'y'))
    for b in range(70):
        _same(dev_pub[b], host_pub[b])
        _same(dev_sec[b], host_sec[b])
        assert [dev_sec[b].seed(n) for n in ('x', 'y')] == [host_sec[b].seed(n) for n in ('x', 'y')]


def test_product_flow_on_device_sampled_inputs(tmp_path):
    """N = 4096 at scale 2^40, the flow of test_gpu_client_batch.py and its 1e-4"""
    compiled, params, sig = _flow(512, 4096, 40)
    xs = _inputs(5, 512, 5)
    pub, sec = generate_keys(params, 5)
    refs = [evaluate(compiled, x) for x in xs]
    for label, encs in (("public", pub.encrypt_batch(xs, sig, device_sampling=True)),
                        ("symmetric", sec.encrypt_batch(xs, sig, device_sampling=True))):
        assert all(e.is_resident(n) for e in encs for n in e.names())
        outs = pub.execute_batch(compiled, encs)
        got = sec.decrypt_batch(outs, sig)
        for b in range(len(xs)):
            for n in refs[b]:
                err = np.abs(np.array(got[b][n]) - np.array(refs[b][n])).max()
                print(f"{label}: instance {b}, output {n}: max error {err:.3g}")
                assert err < 1e-4, (label, b, n)
        _same(outs[0], oracle_execute(pub, compiled, encs[0]))   # the oracle's walk over the same input words
    # a seeded value still saves in its compressed form (c0 + seed), with identical words after load
    pfile, sfile = str(tmp_path / "p.sealvals"), str(tmp_path / "s.sealvals")
    save(pub.encrypt_batch(xs[:1], sig, device_sampling=True)[0], pfile)
    save(encs[1], sfile)
    back = load(sfile)
    for n in back.names():
        assert back.seed(n) == encs[1].seed(n) is not None and back.on_host(n)
    _same(back, encs[1])
    assert (tmp_path / "s.sealvals").stat().st_size <= 0.55 * (tmp_path / "p.sealvals").stat().st_size


def test_the_option_keeps_the_polynomials_off_pcie():
    compiled, params, sig = _flow(8, 1024, 30)
    N, xs = 1024, _inputs(9, 8, 2)
    B = len(xs) * 2   # encrypted values per call: 9 instances of x and of y
    pub, sec = generate_keys(params, 6)
    calls = {
        "public host": lambda: pub.encrypt_batch(xs, sig),
        "public device": lambda: pub.encrypt_batch(xs, sig, device_sampling=True),
        "symmetric host": lambda: sec.encrypt_batch(xs, sig),
        "symmetric device": lambda: sec.encrypt_batch(xs, sig, device_sampling=True),
    }
    sent = {}
    for name, call in calls.items():   # one warm-up call of each kind: keys and tables are on the device afterwards
        call()
    for name, call in calls.items():
        before = pub.transfer_stats()
        call()
        after = pub.transfer_stats()
        sent[name] = after["h2d_bytes"] - before["h2d_bytes"]
        assert after["ct_uploads"] == before["ct_uploads"] and after["d2h_bytes"] == before["d2h_bytes"], name
    print(sent)
    assert sent["public host"] - sent["public device"] == 3 * B * N - 32 * B, sent
    assert sent["symmetric host"] - sent["symmetric device"] == B * N - 32 * B, sent
    assert sent["public device"] == B * (8 * 8 + 32) and sent["symmetric device"] == B * (8 * 8 + 32 + 32), sent
