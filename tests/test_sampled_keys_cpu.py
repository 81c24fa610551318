"""CPU: the whole key set from 32-byte randomness keys, host twin.  generate_keys(..., device_sampling=True)
draws one 32-byte key per polynomial — secret stream: rk_s, ek_pk, one error key per digit of every evaluation key in key
order; public stream: seed_pk, one seed per digit — and expands them with sampled_small / seeded_limb.  The derivation is
restated here from the two test streams alone, the secret key, the public key and every evaluation key are checked against
the key equation in Python integers with the errors sampled_small gives, and the result is an ordinary compressed context
for save, load and format="seal".  The device's key set is compared with this twin in tests/test_gpu_sampled_keygen.py."""
import numpy as np
import pytest

from eva import save, load
from eva.seal import generate_keys
from eva_amd import backend
from sampled_keys import SHAPES, check_key_pair, key_order, keys_of, params_of, stream_keys

SEED = 7


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    """the host twin on every machine, with or without a GPU"""
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


_PAIRS = {}


def _pair(name):
    if name not in _PAIRS:
        _PAIRS[name] = generate_keys(params_of(name), SEED, device_sampling=True)
    return _PAIRS[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_key_equation_with_the_sampled_errors(name):
    pub, sec = _pair(name)
    assert pub.keys_compressed
    check_key_pair(pub, sec, sec._key_randomness())


@pytest.mark.parametrize("name", list(SHAPES))
def test_every_key_is_where_the_contract_puts_it_in_its_stream(name):
    """the order of DESIGN.md 1.8 from the two test streams, restated with the numpy ChaCha20: nothing else is drawn"""
    pub, sec = _pair(name)
    rand, seeds = sec._key_randomness(), pub.key_seeds()
    order = key_order(name)
    D = len(pub.primes) - 1
    assert sorted(order) == sorted(seeds)
    secret = stream_keys(SEED, 1, 2 + len(order) * D)
    public = stream_keys(SEED, 2, 1 + len(order) * D)
    assert rand["secret"] == secret[0] and rand["public"] == secret[1]
    for j, elt in enumerate(order):
        for J in range(D):
            assert rand[elt][J].tobytes() == secret[2 + j * D + J], f"error key of key {elt}, digit {J}"
            assert seeds[elt][J].tobytes() == public[1 + j * D + J], f"seed of key {elt}, digit {J}"
    # seed_pk: the public key's a is its expansion
    from test_seeded_cpu import expand_limb
    pk = pub.public_key()
    for i, q in enumerate(pub.primes):
        assert np.array_equal(pk[1, i], expand_limb(public[0], i, q, pub.poly_modulus_degree)), f"a of the public key, prime {i}"
    # all seeds and all error keys pairwise distinct
    every = [rand["secret"], rand["public"], public[0]]
    for elt in order:
        every += [rand[elt][J].tobytes() for J in range(D)] + [seeds[elt][J].tobytes() for J in range(D)]
    assert len(set(every)) == len(every) == 3 + 2 * len(order) * D


def test_same_seed_same_bytes_other_seed_other_bytes(tmp_path):
    p = params_of("N1024_mixed")
    files = []
    for i, seed in enumerate((SEED, SEED, SEED + 1)):
        pub, _ = generate_keys(p, seed, device_sampling=True)
        path = tmp_path / f"{i}.sealpub"
        save(pub, str(path))
        files.append(path.read_bytes())
    assert files[0] == files[1] and files[0] != files[2]
    # the option changes every draw: not the keys of compress_keys for the same seed
    other, _ = generate_keys(p, SEED, compress_keys=True)
    assert not np.array_equal(other.public_key(), _pair("N1024_mixed")[0].public_key())


@pytest.mark.parametrize("fmt", [None, "seal"])
def test_save_load_round_trip(tmp_path, fmt):
    pub, _ = _pair("N1024_mixed")
    path = str(tmp_path / "ctx")
    save(pub, path, **({"format": fmt} if fmt else {}))
    back = load(path)
    assert back.keys_compressed == (fmt is None)
    k0, k1 = keys_of(pub), keys_of(back)
    assert sorted(k0) == sorted(k1) and all(np.array_equal(k0[e], k1[e]) for e in k0)
    assert np.array_equal(back.public_key(), pub.public_key())
    if fmt is None:
        s0, s1 = pub.key_seeds(), back.key_seeds()
        assert all(np.array_equal(s0[e], s1[e]) for e in s0)


def test_host_twin_holds_its_c0():
    pub, _ = _pair("N1024_mixed")
    N, k = pub.poly_modulus_degree, len(pub.primes)
    assert pub.key_host_bytes() == len(pub.key_seeds()) * (k - 1) * k * N * 8
    full, _ = generate_keys(params_of("N1024_mixed"), SEED)
    assert full.key_host_bytes() == 2 * pub.key_host_bytes()


def test_no_randomness_is_kept_without_a_test_seed():
    _, sec = generate_keys(params_of("N2048_topbit"), 0, device_sampling=True)
    assert sec._key_randomness() == {}
    _, sec = generate_keys(params_of("N2048_topbit"), SEED, compress_keys=True)
    assert sec._key_randomness() == {}


def test_device_path_raises_without_a_device():
    """EVA_DEVICE_CLIENT=0 (the fixture) keeps the client on the host whatever the machine has"""
    with pytest.raises(RuntimeError, match="device_keygen needs a HIP device"):
        generate_keys(params_of("N1024_mixed"), SEED, device_keygen=True, device_sampling=True)
    assert backend.KEY_RELIN == 0
