"""Execution backend (reference: /root/reference/python/eva/seal/__init__.py).  The names are the
reference's; the evaluator behind execute() is the MI355X library libeva_hip.so."""
import numpy as _np

from .._eva import Type as _Type
from .._eva._seal import *  # noqa: F401,F403
from .._eva._seal import SEALPublic as _SEALPublic, SEALSecret as _SEALSecret

# the array types that cross to the device as they are; everything else becomes float64 first
ARRAY_DTYPES = (_np.dtype(_np.uint8), _np.dtype(_np.float32), _np.dtype(_np.float64))


def normalise_arrays(arrays, signature):
    """The arguments of encrypt_array as the library takes them: ({encrypted name: C-contiguous [B, n] array}, {other
    name: list of floats}, B).  An encrypted input of the signature is an array [B, n] with n the signature's vector
    size and one B for every name; a C-contiguous uint8, float32 or float64 array is kept as it is (no copy), anything
    else goes through np.ascontiguousarray(x, dtype=np.float64).  Every other input is one value of n reals shared by
    all instances."""
    n = signature.vec_size
    enc, shared, B, first = {}, {}, None, None
    for name in sorted(arrays):
        if name not in signature.inputs:
            raise KeyError(f"No input named {name} in the signature")
        x = arrays[name]
        if signature.inputs[name].input_type != _Type.Cipher:
            v = _np.asarray(x, dtype=_np.float64)
            if v.ndim != 1:
                raise ValueError(f"input {name} is not encrypted: it is one value of {n} reals shared by all instances, not an array of shape {v.shape}")
            if v.shape[0] != n:
                raise ValueError(f"Input size does not match program vector size (input {name}: {v.shape[0]} values, vector size {n})")
            shared[name] = v.tolist()
            continue
        a = _np.asarray(x)
        if a.dtype not in ARRAY_DTYPES or not a.flags["C_CONTIGUOUS"]:
            a = _np.ascontiguousarray(a, dtype=_np.float64)
        if a.ndim != 2:
            raise ValueError(f"encrypted input {name} needs an array [B, n], one row per instance, not shape {a.shape}")
        if a.shape[1] != n:
            raise ValueError(f"Input size does not match program vector size (input {name}: rows of {a.shape[1]} values, vector size {n})")
        if B is None:
            B, first = a.shape[0], name
        elif a.shape[0] != B:
            raise ValueError(f"input {name} has {a.shape[0]} instances, {first} has {B}")
        enc[name] = a
    if B is None:
        raise ValueError("encrypt_array: no encrypted input array was given")
    if B < 1:
        raise ValueError(f"input {first} has no instances")
    return enc, shared, B


def normalise_plain_arrays(plain_arrays, signature, B):
    """The plain_arrays of encrypt_array as the library takes them: {name: C-contiguous [B, n] array} for
    unencrypted (Raw) inputs of the signature, one row per instance, with n the signature's vector size and B the
    encrypted arrays' B; dtypes as normalise_arrays treats them (uint8, float32, float64 kept, anything else float64)."""
    n = signature.vec_size
    out = {}
    for name in sorted(plain_arrays or {}):
        if name not in signature.inputs:
            raise KeyError(f"No input named {name} in the signature")
        if signature.inputs[name].input_type != _Type.Raw:
            raise ValueError(f"plain_arrays takes unencrypted inputs of type Raw: input {name} is not one")
        a = _np.asarray(plain_arrays[name])
        if a.dtype not in ARRAY_DTYPES or not a.flags["C_CONTIGUOUS"]:
            a = _np.ascontiguousarray(a, dtype=_np.float64)
        if a.ndim != 2:
            raise ValueError(f"unencrypted input {name} in plain_arrays needs an array [B, n], one row per instance, not shape {a.shape}")
        if a.shape[1] != n:
            raise ValueError(f"Input size does not match program vector size (input {name}: rows of {a.shape[1]} values, vector size {n})")
        if a.shape[0] != B:
            raise ValueError(f"input {name} has {a.shape[0]} instances, the encrypted inputs have {B}")
        out[name] = a
    return out


def _encrypt_array(self, arrays, signature, seed=0, plain_arrays=None):
    """encrypt_batch(rows, signature, device_sampling=True, seed=seed) for arrays: `arrays` maps every
    encrypted input to an array [B, n] — uint8, float32 and float64 cross PCIe in their own type and are converted on
    the GPU — and every other input to the one value all instances share.  Returns a SEALValuationBatch whose instance b
    is encrypt_batch's instance b word for word; per name the instances stay in batched handles of at most 64.
    Raises without a HIP device, with EVA_DEVICE_CLIENT=0, with resident = False and for a value the device encoder
    cannot take: there is no host path behind this call.
    plain_arrays: {name: array [B, n]} for unencrypted (Raw) inputs that differ per instance, kept in
    their own type; execute_batch encodes a group's rows on the device where the program encodes the input."""
    enc, shared, B = normalise_arrays(arrays, signature)
    plains = normalise_plain_arrays(plain_arrays, signature, B)
    for name in plains:
        if name in shared:
            raise ValueError(f"input {name} is given twice: in arrays and in plain_arrays")
    return self._encrypt_array(enc, shared, signature, seed, plains)


_SEALPublic.encrypt_array = _encrypt_array
_SEALSecret.encrypt_array = _encrypt_array
