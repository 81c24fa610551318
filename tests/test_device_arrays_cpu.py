"""CPU: the argument side of encrypt_array on device arrays, the part that needs no GPU.
eva.seal.normalise_device_arrays on objects that carry only a __cuda_array_interface__ dict: every accepted form — the
three types, contiguous and pitched rows, a stream entry, an explicit stream — and every refusal with its message.  Where
no device is visible a device array raises encrypt_array's error instead of going through the host, and decrypt_array
still refuses a dtype it has no rule for."""
import numpy as np
import pytest

from eva.seal import generate_keys, is_device_array, normalise_device_arrays
from eva_amd import backend
from test_client_array_cpu import W, _program


class Fake:
    """device memory as far as the interface goes: nothing here is ever dereferenced"""

    def __init__(self, shape, typestr, strides=None, ptr=0x7f0000001000, **extra):
        self.__cuda_array_interface__ = dict({"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}, **extra)


@pytest.fixture(scope="module")
def sig():
    return _program()[2]


def test_what_counts_as_a_device_array():
    assert is_device_array(Fake((5, 64), "|u1"))
    assert not is_device_array(np.zeros((5, 64)))
    assert not is_device_array([[0.0] * 64] * 5)

    class Raises:
        @property
        def __cuda_array_interface__(self):   # (a torch CPU tensor answers like this)
            raise TypeError("not a device tensor")
    assert not is_device_array(Raises())


@pytest.mark.parametrize("typestr,code,item", [("|u1", backend.U8, 1), ("<f4", backend.F32, 4), ("<f8", backend.F64, 8)])
def test_accepted_forms(sig, typestr, code, item):
    x = Fake((5, 64), typestr)
    y = Fake((5, 64), typestr, strides=(64 * item + 3 * item, item), ptr=0x7f0000002000 + item)
    out, B, first = normalise_device_arrays({'x': x, 'y': y}, sig)
    assert B == 5 and first == 'x'
    assert out['x'] == (0x7f0000001000, code, 5, 64, 64 * item, 0)                 # strides None: contiguous, no stream
    assert out['y'] == (0x7f0000002000 + item, code, 5, 64, 67 * item, 0)          # pitched rows
    # contiguous strides spelled out, and a single row whose outer stride means nothing
    assert normalise_device_arrays({'x': Fake((5, 64), typestr, strides=(64 * item, item))}, sig)[0]['x'][4] == 64 * item
    assert normalise_device_arrays({'x': Fake((1, 64), typestr, strides=(0, item))}, sig)[0]['x'][2:5] == (1, 64, 64 * item)


def test_streams(sig):
    x = lambda **kw: {'x': Fake((2, 64), "<f4", **kw)}
    assert normalise_device_arrays(x(), sig)[0]['x'][5] == 0                        # nothing known: the caller synchronised
    assert normalise_device_arrays(x(stream=None), sig)[0]['x'][5] == 0
    assert normalise_device_arrays(x(stream=1), sig)[0]['x'][5] == 1                # the interface's entry: the null stream
    assert normalise_device_arrays(x(stream=0x5500), sig)[0]['x'][5] == 0x5500
    assert normalise_device_arrays(x(stream=0x5500), sig, stream=0x6600)[0]['x'][5] == 0x6600   # the argument wins

    class S:
        cuda_stream = 0x7700
    assert normalise_device_arrays(x(), sig, stream=S())[0]['x'][5] == 0x7700
    S.cuda_stream = 0                                                               # torch's name for the null stream
    assert normalise_device_arrays(x(), sig, stream=S())[0]['x'][5] == 1


def test_refusals_say_what_to_convert(sig):
    ok = Fake((5, 64), "<f4")
    cases = [
        (Fake((64,), "<f4"), r"encrypted input x needs a device array \[B, n\].*not shape \(64,\)"),
        (Fake((5, 8, 8), "<f4"), r"encrypted input x needs a device array \[B, n\]"),
        (Fake((5, 64), "<i4"), r"input x: a device array must be uint8, float32 or float64 .*not <i4"),
        (Fake((5, 64), ">f8"), r"input x: a device array must be uint8, float32 or float64 .*not >f8"),
        (Fake((5, 64), "<f4", strides=(512, 8)), r"input x: the values of a row must be adjacent \(inner stride 8, item size 4\).*contiguous"),
        (Fake((5, 64), "<f4", strides=(128, 4)), r"input x: row stride 128 must be a multiple of the item size 4 and at least a row \(256 bytes\)"),
        (Fake((5, 64), "<f4", strides=(258, 4)), r"input x: row stride 258 must be a multiple of the item size 4"),
        (Fake((5, 64), "|u1", mask=Fake((5, 64), "|u1")), r"input x: a masked device array is not supported"),
        (Fake((5, 64), "<f4", ptr=0), r"input x: the device array has no data"),
        (Fake((5, 63), "<f4"), r"Input size does not match program vector size \(input x: rows of 63 values, vector size 64\)"),
        (Fake((0, 64), "<f4"), r"input x has no instances"),
    ]
    for x, message in cases:
        with pytest.raises(ValueError, match=message):
            normalise_device_arrays({'x': x}, sig)
    with pytest.raises(ValueError, match="input y has 4 instances, x has 5"):
        normalise_device_arrays({'x': ok, 'y': Fake((4, 64), "|u1")}, sig)
    with pytest.raises(ValueError, match="input w is not encrypted"):
        normalise_device_arrays({'x': ok, 'w': Fake((5, 64), "<f8")}, sig)
    with pytest.raises(KeyError, match="No input named q"):
        normalise_device_arrays({'q': ok}, sig)


def test_encrypt_array_checks_device_arrays_before_it_needs_a_device(monkeypatch):
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 3)
    dev = Fake((3, 64), "|u1")
    host = np.ones((3, 64), dtype=np.float32)
    for ctx in (pub, sec):
        # the argument checks come first, with or without a device: B across host and device names, plain_arrays on the host
        with pytest.raises(ValueError, match="input y has 2 instances, x has 3"):
            ctx.encrypt_array({'x': dev, 'y': host[:2], 'w': W}, sig)
        with pytest.raises(ValueError, match="input y has 2 instances, x has 3"):
            ctx.encrypt_array({'x': dev, 'y': Fake((2, 64), "<f8"), 'w': W}, sig)
        with pytest.raises(ValueError, match="plain_arrays stays on the host: input w is a device array"):
            ctx.encrypt_array({'x': dev, 'y': host}, sig, plain_arrays={'w': Fake((3, 64), "<f8")})
        with pytest.raises(ValueError, match="a device array must be uint8, float32 or float64"):
            ctx.encrypt_array({'x': Fake((3, 64), "<f2"), 'y': host, 'w': W}, sig)
    if backend.device_count() == 0:
        for ctx in (pub, sec):
            with pytest.raises(RuntimeError, match="encrypt_array needs a HIP device"):
                ctx.encrypt_array({'x': dev, 'y': host, 'w': W}, sig)
            with pytest.raises(RuntimeError, match="encrypt_array needs a HIP device"):
                ctx.encrypt_array({'x': dev, 'y': Fake((3, 64), "<f8"), 'w': W}, sig, stream=0x5500)
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    pub0, sec0 = generate_keys(params, 3)
    for ctx in (pub0, sec0):
        with pytest.raises(RuntimeError, match="EVA_DEVICE_CLIENT=0 keeps the client on the host"):
            ctx.encrypt_array({'x': dev, 'y': host, 'w': W}, sig, seed=4)


def test_decrypt_array_still_refuses_other_dtypes():
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 3)
    for dtype in (np.int16, np.float16, np.int8, np.uint16):
        with pytest.raises(ValueError, match="decrypt_array: dtype must be float64, float32 or uint8"):
            sec.decrypt_array([], sig, dtype=dtype)
        with pytest.raises(ValueError, match="decrypt_array: dtype must be float64, float32 or uint8"):
            sec.decrypt_array([], sig, dtype=dtype, device=True)
    if backend.device_count() == 0:
        for kw in ({"dtype": np.uint8}, {"device": True}):
            with pytest.raises(RuntimeError, match="decrypt_array needs a HIP device"):
                sec.decrypt_array([], sig, **kw)
