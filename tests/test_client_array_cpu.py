"""CPU: the argument side of encrypt_array, the part that needs no GPU.  eva.seal.normalise_arrays:
which arrays cross as they are (C-contiguous uint8 / float32 / float64, without a copy) and which become float64 first,
the shape checks by name, and a non-encrypted input as one shared value.  Where no device is visible encrypt_array raises
instead of computing on the host; test_cabi_symbols.py covers the new declarations."""
import numpy as np
import pytest

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys, normalise_arrays
from eva_amd import backend


def _program(vec=64, N=2048):
    prog = EvaProgram('arrays', vec_size=vec)
    with prog:
        x, y, w = Input('x'), Input('y'), Input('w', False)
        Output('z', x * y + w)
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    params.poly_modulus_degree = N
    return compiled, params, sig


@pytest.fixture(scope="module")
def sig():
    return _program()[2]


W = [0.5] * 64


@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64])
def test_the_three_types_cross_as_they_are(sig, dtype):
    x = np.arange(5 * 64).reshape(5, 64).astype(dtype)
    y = np.ones((5, 64), dtype=dtype)
    enc, shared, B = normalise_arrays({'x': x, 'y': y, 'w': W}, sig)
    assert B == 5 and sorted(enc) == ['x', 'y'] and shared == {'w': W}
    assert enc['x'] is x and enc['y'] is y          # no copy, no conversion
    assert enc['x'].dtype == np.dtype(dtype)


def test_everything_else_becomes_contiguous_float64(sig):
    base = np.arange(5 * 128, dtype=np.float32).reshape(5, 128)
    cases = {
        "int64": np.arange(5 * 64, dtype=np.int64).reshape(5, 64),
        "float16": np.ones((5, 64), dtype=np.float16),
        "bool": np.ones((5, 64), dtype=bool),
        "strided float32": base[:, ::2],
        "transposed uint8": np.ones((64, 5), dtype=np.uint8).T,
        "lists": [[float(i)] * 64 for i in range(5)],
    }
    for label, x in cases.items():
        enc, _, B = normalise_arrays({'x': x, 'y': np.zeros((5, 64)), 'w': W}, sig)
        a = enc['x']
        assert B == 5 and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] and a.shape == (5, 64), label
        assert np.array_equal(a, np.asarray(x, dtype=np.float64)), label
    # mixed types in one call: each array keeps its own
    enc, _, _ = normalise_arrays({'x': np.zeros((2, 64), dtype=np.uint8), 'y': np.zeros((2, 64), dtype=np.float32), 'w': W}, sig)
    assert enc['x'].dtype == np.uint8 and enc['y'].dtype == np.float32


def test_shape_errors_name_the_input(sig):
    ok = np.zeros((5, 64), dtype=np.float32)
    with pytest.raises(ValueError, match=r"Input size does not match program vector size \(input y"):
        normalise_arrays({'x': ok, 'y': np.zeros((5, 63), dtype=np.float32), 'w': W}, sig)
    with pytest.raises(ValueError, match="input y has 4 instances, x has 5"):
        normalise_arrays({'x': ok, 'y': ok[:4], 'w': W}, sig)
    with pytest.raises(ValueError, match=r"encrypted input x needs an array \[B, n\]"):
        normalise_arrays({'x': ok[0], 'y': ok, 'w': W}, sig)
    with pytest.raises(KeyError, match="No input named q"):
        normalise_arrays({'x': ok, 'y': ok, 'w': W, 'q': ok}, sig)
    with pytest.raises(ValueError, match="no encrypted input array"):
        normalise_arrays({'w': W}, sig)
    with pytest.raises(ValueError, match="input x has no instances"):
        normalise_arrays({'x': ok[:0], 'y': ok[:0], 'w': W}, sig)


def test_a_non_encrypted_input_is_one_shared_value(sig):
    ok = np.zeros((5, 64), dtype=np.uint8)
    _, shared, _ = normalise_arrays({'x': ok, 'y': ok, 'w': np.arange(64, dtype=np.int32)}, sig)
    assert shared == {'w': [float(i) for i in range(64)]}
    with pytest.raises(ValueError, match="input w is not encrypted: it is one value"):
        normalise_arrays({'x': ok, 'y': ok, 'w': np.zeros((5, 64))}, sig)
    with pytest.raises(ValueError, match=r"Input size does not match program vector size \(input w"):
        normalise_arrays({'x': ok, 'y': ok, 'w': [0.5] * 63}, sig)


def test_no_host_path_behind_encrypt_array(monkeypatch):
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 3)
    arrays = {'x': np.ones((3, 64), dtype=np.uint8), 'y': np.ones((3, 64), dtype=np.float32), 'w': W}
    if backend.device_count() == 0:
        for ctx in (pub, sec):
            with pytest.raises(RuntimeError, match="encrypt_array needs a HIP device"):
                ctx.encrypt_array(arrays, sig)
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    pub0, sec0 = generate_keys(params, 3)
    for ctx in (pub0, sec0):
        with pytest.raises(RuntimeError, match="EVA_DEVICE_CLIENT=0 keeps the client on the host"):
            ctx.encrypt_array(arrays, sig, seed=4)
    # the argument checks come first, with or without a device
    with pytest.raises(ValueError, match="input y has 2 instances"):
        pub0.encrypt_array(dict(arrays, y=arrays['y'][:2]), sig)
