"""CPU: evaluation keys generated on the GPU, the part that needs none.  evah_keygen_switch is declared
and exported; generate_keys(..., device_keygen=True) refuses to fall back to the host generator; the host generator,
whose draws now go through the one place the device path shares (KeyGenerator::draw_seeded_digit), still produces the
words it produced before — compared with digests recorded from the commit before the refactor — and the container of a
compressed context is unchanged."""
import hashlib
import os
import re
import struct

import numpy as np
import pytest

from eva import save
from eva.ckks import CKKSParameters
from eva.seal import generate_keys
from eva_amd import backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the shapes of tests/test_gpu_keygen.py
SHAPES = {
    "N1024_mixed": (1024, [60, 30, 45, 50, 33, 60], (1, -3, 0)),
    "N2048_topbit": (2048, [60, 50, 50, 60], (5,)),
    "N1024_17digits": (1024, [30] * 16 + [31, 31], (2,)),
}

# sha256 over (secret key, public key, relinearization key, Galois keys by element[, seeds in the same order]) of
# generate_keys(params, 7[, compress_keys=True]) at the commit before the draw order was factored out
PARENT_DIGESTS = {
    "N1024_mixed": ("538ac7ef17c38a5f7eda959a0b6e585ab3fd2eb76752832b80f8b381cefd2204", "ca435479226324e0e3607c75f3d5bca1ab931d835887ef11f1d03c8f37c027ce"),
    "N2048_topbit": ("b8f8374c76760572eb4bc98aa6b524a89c6f0731fc81f1760b8065b62fac556f", "b0b1b7d19fa725f0ddcbf9fbd4b3a0d88b650b4f0943d7c4606082fcaa683e08"),
    "N1024_17digits": ("8c327c823fad7db8b5cec16d4701f595078665b4be78fa192d4e1e473c024435", "dcd21d0ed686ac89c82ed0606cada5c9554b0f19ed7406da6d4fb9bdef086b28"),
}


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    """the host client on every machine, with or without a GPU (tests/test_gpu_keygen.py covers the device)"""
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


def _params(name):
    N, bits, steps = SHAPES[name]
    return CKKSParameters(list(bits), set(steps), N)


def _digest(pub, sec):
    h = hashlib.sha256()
    keys = {0: pub.relin_key()}
    keys.update(pub.galois_keys())
    for a in [sec._secret_key_ntt(), pub.public_key()] + [keys[e] for e in sorted(keys)]:
        h.update(np.ascontiguousarray(a, dtype="<u8").tobytes())
    seeds = pub.key_seeds()
    if seeds is not None:
        assert sorted(seeds) == sorted(keys)
        for e in sorted(seeds):
            h.update(np.ascontiguousarray(seeds[e], dtype=np.uint8).tobytes())
    return h.hexdigest()


def test_entry_point_is_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "eva_hip.h")).read()
    decl = re.search(r"int evah_keygen_switch\(([^;]*)\);", header)
    assert decl, "evah_keygen_switch is not declared in include/eva_hip.h"
    args = re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S)
    assert [a.split()[-1].lstrip("*") for a in args.split(",")] == ["ctx", "kind", "galois_elt", "n_digits", "errors", "seeds", "install", "c0_out"]
    assert "seal.cpp:174-203" in header[:decl.start()].rsplit("/*", 1)[1]   # the comment on the declaration cites generateKeys
    lib = backend.load()
    assert hasattr(lib, "evah_keygen_switch")
    assert hasattr(backend.Context, "keygen_switch")
    # the counter that tells an uploaded key from one generated in place
    assert re.search(r"int evah_ctx_key_upload_stats\(evah_ctx \*ctx, uint64_t out\[2\]\);", header)
    assert hasattr(lib, "evah_ctx_key_upload_stats") and hasattr(backend.Context, "key_upload_stats")


def test_device_keygen_without_a_device_is_an_error_not_a_fallback():
    """EVA_DEVICE_CLIENT=0 (set for this file), or no HIP device at all: the option raises, it does not quietly run the
    host generator"""
    with pytest.raises(RuntimeError, match="device_keygen needs a HIP device"):
        generate_keys(_params("N2048_topbit"), 7, device_keygen=True)
    # the option off: nothing changes
    pub, _ = generate_keys(_params("N2048_topbit"), 7)
    assert not pub.keys_compressed


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_generator_draws_what_it_drew_before(name):
    p = _params(name)
    pub0, sec0 = generate_keys(p, 7)
    pubc, secc = generate_keys(p, 7, compress_keys=True)
    assert not pub0.keys_compressed and pubc.keys_compressed
    # the secret and the public key do not depend on the option
    assert np.array_equal(sec0._secret_key_ntt(), secc._secret_key_ntt())
    assert np.array_equal(pub0.public_key(), pubc.public_key())
    full, comp = PARENT_DIGESTS[name]
    assert _digest(pub0, sec0) == full, "uncompressed keys differ from the words generated before the refactor"
    assert _digest(pubc, secc) == comp, "compressed keys differ from the words generated before the refactor"
    # and a second call with the same seed gives them again
    assert _digest(*generate_keys(p, 7)) == full
    assert _digest(*generate_keys(p, 7, compress_keys=True)) == comp


def test_compressed_file_layout_is_unchanged(tmp_path):
    """the container of a compressed context, restated field by field from key_seeds() / relin_key(): N, primes, public
    key, then per key the flagged digit count, the seeds (length, bytes) and c0 (length, words)"""
    N = SHAPES["N1024_mixed"][0]
    pub, _ = generate_keys(_params("N1024_mixed"), 7, compress_keys=True)
    path = tmp_path / "c.sealpub"
    save(pub, str(path))
    primes, seeds = pub.primes, pub.key_seeds()
    k, D = len(primes), len(primes) - 1

    def key(words, sd):
        c0 = np.ascontiguousarray(words[:, 0])
        assert sd.shape == (D, 32) and c0.shape == (D, k, N)
        return struct.pack("<IQ", D | 0x80000000, 32 * D) + sd.tobytes() + struct.pack("<Q", c0.size) + c0.astype("<u8").tobytes()
    want = struct.pack("<III", 0x48415645, 1, 5) + struct.pack("<I", N) + struct.pack("<Q", k) + np.array(primes, dtype="<u8").tobytes()
    want += struct.pack("<Q", 2 * k * N) + pub.public_key().astype("<u8").tobytes()
    want += key(pub.relin_key(), seeds[0])
    gk = pub.galois_keys()
    assert len(gk) == 3
    want += struct.pack("<Q", len(gk))
    for elt in sorted(gk):
        want += struct.pack("<I", elt) + key(gk[elt], seeds[elt])
    assert path.read_bytes() == want
