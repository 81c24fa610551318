"""CPU: the argument side of encrypt_array(..., plain_arrays=...), the part that needs no GPU.
eva.seal.normalise_plain_arrays: an unencrypted (Raw) input as an array [B, n] with a row per instance — which dtypes
cross as they are, what is converted, and the shape checks by name — and normalise_arrays with its two arguments as it
was.  test_cabi_symbols.py covers the new declarations of the header."""
import numpy as np
import pytest

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys, normalise_arrays, normalise_plain_arrays
from eva_amd import backend


def _program(vec=64, N=2048):
    prog = EvaProgram('plain_rows', vec_size=vec)
    with prog:
        x, y, w = Input('x'), Input('y'), Input('w', False)
        Output('z', x * w + y)
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    params.poly_modulus_degree = N
    return compiled, params, sig


@pytest.fixture(scope="module")
def sig():
    return _program()[2]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_the_three_types_are_kept(sig, dtype):
    w = np.arange(5 * 64).reshape(5, 64).astype(dtype)
    out = normalise_plain_arrays({'w': w}, sig, 5)
    assert list(out) == ['w'] and out['w'] is w and out['w'].dtype == np.dtype(dtype)   # no copy, no conversion


def test_everything_else_becomes_contiguous_float64(sig):
    base = np.arange(5 * 128, dtype=np.float32).reshape(5, 128)
    cases = {
        "int64": np.arange(5 * 64, dtype=np.int64).reshape(5, 64),
        "float16": np.ones((5, 64), dtype=np.float16),
        "strided float32": base[:, ::2],
        "transposed uint8": np.ones((64, 5), dtype=np.uint8).T,
        "lists": [[float(i)] * 64 for i in range(5)],
    }
    for label, w in cases.items():
        a = normalise_plain_arrays({'w': w}, sig, 5)['w']
        assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.shape == (5, 64), label
        assert np.array_equal(a, np.asarray(w, dtype=np.float64)), label


def test_nothing_given_is_nothing(sig):
    assert normalise_plain_arrays(None, sig, 5) == {} and normalise_plain_arrays({}, sig, 5) == {}


def test_errors_name_the_input(sig):
    ok = np.zeros((5, 64), dtype=np.float32)
    with pytest.raises(ValueError, match=r"unencrypted input w in plain_arrays needs an array \[B, n\]"):
        normalise_plain_arrays({'w': ok[0]}, sig, 5)
    with pytest.raises(ValueError, match=r"unencrypted input w in plain_arrays needs an array \[B, n\]"):
        normalise_plain_arrays({'w': ok[None]}, sig, 5)
    with pytest.raises(ValueError, match=r"Input size does not match program vector size \(input w: rows of 63"):
        normalise_plain_arrays({'w': np.zeros((5, 63))}, sig, 5)
    with pytest.raises(ValueError, match="input w has 4 instances, the encrypted inputs have 5"):
        normalise_plain_arrays({'w': ok[:4]}, sig, 5)
    with pytest.raises(ValueError, match="plain_arrays takes unencrypted inputs of type Raw: input x is not one"):
        normalise_plain_arrays({'x': ok}, sig, 5)
    with pytest.raises(KeyError, match="No input named q"):
        normalise_plain_arrays({'q': ok}, sig, 5)


def test_normalise_arrays_with_two_arguments_is_unchanged(sig):
    ok = np.zeros((5, 64), dtype=np.uint8)
    W = [0.5] * 64
    enc, shared, B = normalise_arrays({'x': ok, 'y': ok, 'w': W}, sig)
    assert B == 5 and enc['x'] is ok and enc['y'] is ok and shared == {'w': W}
    enc, shared, B = normalise_arrays({'x': ok, 'y': ok}, sig)   # w left out here: it may come through plain_arrays
    assert B == 5 and shared == {}
    with pytest.raises(ValueError, match="input w is not encrypted: it is one value of 64 reals shared by all instances, not an array of shape"):
        normalise_arrays({'x': ok, 'y': ok, 'w': np.zeros((5, 64))}, sig)
    with pytest.raises(ValueError, match="input y has 4 instances, x has 5"):
        normalise_arrays({'x': ok, 'y': ok[:4], 'w': W}, sig)


def test_the_checks_come_before_the_device(monkeypatch):
    """encrypt_array makes the plain_arrays checks with or without a device, and refuses a name given both ways"""
    compiled, params, sig = _program()
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    pub, sec = generate_keys(params, 3)
    arrays = {'x': np.ones((3, 64), dtype=np.uint8), 'y': np.ones((3, 64), dtype=np.float32)}
    for ctx in (pub, sec):
        with pytest.raises(ValueError, match="input w has 2 instances, the encrypted inputs have 3"):
            ctx.encrypt_array(arrays, sig, plain_arrays={'w': np.zeros((2, 64))})
        with pytest.raises(ValueError, match="input w is given twice"):
            ctx.encrypt_array(dict(arrays, w=[0.5] * 64), sig, plain_arrays={'w': np.zeros((3, 64))})
        with pytest.raises(RuntimeError, match="EVA_DEVICE_CLIENT=0 keeps the client on the host"):
            ctx.encrypt_array(arrays, sig, seed=4, plain_arrays={'w': np.zeros((3, 64))})
    assert backend.EXPORTED_SYMBOLS.count("evah_pt_encode_array") == 1
