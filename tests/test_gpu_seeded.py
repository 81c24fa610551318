"""GPU: seed-compressed symmetric ciphertexts on the MI355X — the device expansion of c1 against the
numpy ChaCha20 of test_seeded_cpu.py, device encryption against the host's word for word, execute() on seeded inputs
bit-exact against the same ciphertexts uploaded in full (every upload path: resident, host valuations, the graph
plan's slots, execute_batch, sub-DAG and limb sharding), and the PCIe bytes a seeded input saves."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from eva import evaluate, save, load
from eva.ckks import CKKSCompiler
from eva.metric import valuation_mse
from eva.seal import generate_keys, SEALValuation
from eva_amd import backend, workloads
from eva_amd.hostref import coeff_modulus_create
from evatest import oracle_execute
from test_seeded_cpu import expand_limb

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,bits", [(1024, [60, 30, 45, 50, 33, 60]), (1 << 16, [60] + [50] * 9 + [60])])
def test_device_expansion_matches_numpy(N, bits):
    primes = coeff_modulus_create(N, bits)
    L = len(primes) - 1
    ctx = backend.Context(N, primes, device=0)
    rng = random.Random(N)
    seeds = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(3)]
    ct = ctx.upload_ct_seeded(np.zeros((3, L, N), dtype=np.uint64), seeds, 2.0 ** 30)
    got = ct.download()
    assert got.shape == (3, 2, L, N)
    assert not got[:, 0].any()
    for b, seed in enumerate(seeds):
        for i in range(L):
            assert np.array_equal(got[b, 1, i], expand_limb(seed, i, primes[i], N)), f"instance {b}, limb {i}"
    one = ctx.upload_ct_seeded(np.zeros((L, N), dtype=np.uint64), seeds[:1], 2.0 ** 30)
    assert np.array_equal(one.download_poly(1), got[0, 1]) and not one.download_poly(0).any()
    one.free()
    ct.free()
    ctx.close()


def _readme():
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(workloads.readme_polynomial())
    return workloads.readme_polynomial(), compiled, params, sig, {"x": [i / 1024.0 for i in range(1024)]}


def _sobel():
    prog = workloads.sobel(32, 32, 1024)
    prog.set_input_scales(25)
    prog.set_output_ranges(10)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    return prog, compiled, params, sig, workloads.image(1024)


def _materialised(enc):
    mat = SEALValuation()
    for n in enc.names():
        kind, _, _, scale, data = enc.get(n)
        assert kind == "cipher"
        mat._set_cipher(n, data, scale)
    return mat


def _same(a, b):
    assert sorted(a.names()) == sorted(b.names())
    for n in a.names():
        x, y = a.get(n), b.get(n)
        assert x[:4] == y[:4], (n, x[:4], y[:4])
        assert np.array_equal(np.asarray(x[4]), np.asarray(y[4])), f"output {n} differs"


_CHILD = r"""
import sys
from eva import save
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys
from eva_amd import workloads
compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(workloads.readme_polynomial())
pub, sec = generate_keys(params, 7)
enc = sec.encrypt({"x": [i / 1024.0 for i in range(1024)]}, sig, seed=5)
assert not enc.is_resident("x")
save(enc, sys.argv[1])
"""


@pytest.mark.parametrize("encode,resident", [("1", "1"), ("0", "1"), ("1", "0")])
def test_device_encrypt_equals_host(encode, resident, monkeypatch, tmp_path):
    """the device encoder route (evah_pt_encode) and the host encoder + evah_pt_upload_coeff route; resident
    results, and host results whose c0 alone was downloaded"""
    monkeypatch.setenv("EVA_DEVICE_ENCODE", encode)
    monkeypatch.setenv("EVA_RESIDENT", resident)
    path = str(tmp_path / "host.sealvals")
    env = dict(os.environ, PYTHONPATH=ROOT, EVA_DEVICE_CLIENT="0", EVA_RESIDENT="1", EVA_DEVICE_ENCODE="1")
    out = subprocess.run([sys.executable, "-c", _CHILD, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    host = load(path)
    _, _, params, sig, inputs = _readme()
    pub, sec = generate_keys(params, 7)
    dev = sec.encrypt(inputs, sig, seed=5)
    assert dev.is_resident("x") == (resident == "1") and dev.on_host("x") == (resident == "0")
    assert dev.seed("x") == host.seed("x")
    _same(dev, host)


@pytest.mark.parametrize("mode", ["resident", "host", "subdag", "limb"])
def test_execute_on_seeded_inputs_is_bit_exact(mode, monkeypatch, tmp_path):
    if mode == "host":
        monkeypatch.setenv("EVA_RESIDENT", "0")
    kw = {"devices": [0, 0], "shard": mode} if mode in ("subdag", "limb") else {}
    prog, compiled, params, sig, inputs = _readme()
    pub, sec = generate_keys(params, 7, **kw)
    enc = sec.encrypt(inputs, sig, seed=11)
    save(enc, str(tmp_path / "s.sealvals"))
    seeded = load(str(tmp_path / "s.sealvals"))   # c0 + seed on the host: the seeded upload paths
    assert seeded.seed("x") == enc.seed("x") and seeded.on_host("x") and not seeded.is_resident("x")
    mat = _materialised(enc)
    want = oracle_execute(pub, compiled, mat)
    _same(pub.execute(compiled, mat), want)
    for call in range(3):   # eager walk, plan capture (slot upload + refill), replay (seeded slot refill)
        _same(pub.execute(compiled, seeded), want)
    for call in range(2):   # the encrypt() result itself (resident unless EVA_RESIDENT=0)
        out = pub.execute(compiled, enc)
        _same(out, want)
    assert valuation_mse(sec.decrypt(out, sig), evaluate(prog, inputs)) < 0.01


def test_execute_batch_on_seeded_inputs(monkeypatch, tmp_path):
    monkeypatch.setenv("EVA_RESIDENT", "0")
    prog, compiled, params, sig, _ = _readme()
    pub, sec = generate_keys(params, 7)
    ins = [{"x": [((i * (b + 3)) % 1024) / 1024.0 for i in range(1024)]} for b in range(3)]
    encs = [sec.encrypt(x, sig, seed=40 + b) for b, x in enumerate(ins)]
    assert len({e.seed("x") for e in encs}) == 3
    for e in encs:
        assert e.on_host("x") and not e.is_resident("x")
    outs = pub.execute_batch(compiled, encs)
    for b, e in enumerate(encs):
        _same(outs[b], oracle_execute(pub, compiled, _materialised(e)))
        assert valuation_mse(sec.decrypt(outs[b], sig), evaluate(prog, ins[b])) < 0.01


def test_sobel_on_seeded_inputs():
    prog, compiled, params, sig, inputs = _sobel()
    pub, sec = generate_keys(params, 3)
    enc = sec.encrypt(inputs, sig, seed=2)
    out = pub.execute(compiled, enc)
    _same(out, oracle_execute(pub, compiled, _materialised(enc)))
    assert valuation_mse(sec.decrypt(out, sig), evaluate(prog, inputs)) < 0.01


def test_seeded_inputs_save_their_bytes(monkeypatch):
    """host valuations: the same program on seeded and on public-key inputs, each on a fresh key pair — the
    h2d bytes of one execute() differ by l N 8 - 32 per input (constants upload the same bytes in both)"""
    monkeypatch.setenv("EVA_RESIDENT", "0")
    _, compiled, params, sig, inputs = _readme()
    deltas = {}
    for kind in ("seeded", "public"):
        pub, sec = generate_keys(params, 7)
        enc = sec.encrypt(inputs, sig, seed=3) if kind == "seeded" else pub.encrypt(inputs, sig)
        d = []
        for call in range(3):   # eager walk, capture, replay
            before = pub.transfer_stats()["h2d_bytes"]
            pub.execute(compiled, enc)
            d.append(pub.transfer_stats()["h2d_bytes"] - before)
        deltas[kind] = d
    N = params.poly_modulus_degree
    k = len(params.prime_bits)
    saved = sum((k - 1 - sig.inputs[n].level) * N * 8 - 32 for n in inputs)
    assert deltas["public"][0] - deltas["seeded"][0] == saved, deltas
    assert deltas["public"][2] - deltas["seeded"][2] == saved, deltas
