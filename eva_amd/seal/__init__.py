"""Execution backend (reference: /root/reference/python/eva/seal/__init__.py).  The names are the
reference's; the evaluator behind execute() is the MI355X library libeva_hip.so."""
import sys as _sys

import numpy as _np

from .._eva import Type as _Type
from .._eva._seal import *  # noqa: F401,F403
from .._eva._seal import SEALPublic as _SEALPublic, SEALSecret as _SEALSecret

# the array types that cross to the device as they are; everything else becomes float64 first
ARRAY_DTYPES = (_np.dtype(_np.uint8), _np.dtype(_np.float32), _np.dtype(_np.float64))


def normalise_arrays(arrays, signature, allow_none=False):
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
        if allow_none:   # (the encrypted inputs of this call are all device arrays)
            return enc, shared, None
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


_DEVICE_TYPESTRS = {"|u1": 2, "<f4": 1, "<f8": 0}   # __cuda_array_interface__ typestr -> EVAH_U8 / EVAH_F32 / EVAH_F64


def is_device_array(x):
    """an object that describes device memory through __cuda_array_interface__ (a torch tensor on the GPU, a
    backend.DeviceView, a DeviceArray).  A torch CPU tensor has the attribute and raises from it: it is a host array."""
    if isinstance(x, _np.ndarray):
        return False
    try:
        return isinstance(x.__cuda_array_interface__, dict)
    except Exception:
        return False


def _producer_stream(x, iface, stream):
    """the stream the rows of x were written on, as the library takes it: an address, 1 for the null stream, 0 for none.
    An explicit `stream` (an address, or an object with .cuda_stream) wins over the interface's own entry; a torch tensor
    without either was written on torch's current stream for its device.  torch is looked up, never imported."""
    if stream is not None:
        s = int(getattr(stream, "cuda_stream", stream))
        return s if s else 1   # (torch names the null stream 0)
    if iface.get("stream") is not None:
        return int(iface["stream"])   # (the interface's own numbering: 1 the null stream, 2 the per-thread default)
    torch = _sys.modules.get("torch")
    if torch is not None and isinstance(x, torch.Tensor):
        return int(torch.cuda.current_stream(x.device).cuda_stream) or 1
    return 0


def normalise_device_arrays(arrays, signature, stream=None):
    """The device arrays of encrypt_array as the library takes them: ({name: (device pointer, EVAH_*
    code, B, n, row pitch in bytes, producer stream)}, B, first name) from objects with __cuda_array_interface__.
    Accepted: shape [B, n] with n the signature's vector size; typestr |u1, <f4 or <f8; strides None or (pitch, itemsize)
    with pitch a multiple of the item size and at least a row; no mask; a `stream` entry is honoured.  Anything else
    is refused with what to convert — nothing goes through the host silently."""
    n = signature.vec_size
    out, B, first = {}, None, None
    for name in sorted(arrays):
        if name not in signature.inputs:
            raise KeyError(f"No input named {name} in the signature")
        x = arrays[name]
        if signature.inputs[name].input_type != _Type.Cipher:
            raise ValueError(f"input {name} is not encrypted: it is one value of {n} reals shared by all instances, not a device array")
        iface = x.__cuda_array_interface__
        shape = tuple(int(s) for s in iface["shape"])
        if len(shape) != 2:
            raise ValueError(f"encrypted input {name} needs a device array [B, n], one row per instance, not shape {shape}: reshape it")
        code = _DEVICE_TYPESTRS.get(iface["typestr"])
        if code is None:
            raise ValueError(f"input {name}: a device array must be uint8, float32 or float64 (typestr |u1, <f4, <f8), not {iface['typestr']}: "
                             "convert it on the device first (tensor.to(torch.float32))")
        item = {2: 1, 1: 4, 0: 8}[code]
        if iface.get("mask") is not None:
            raise ValueError(f"input {name}: a masked device array is not supported: materialise the values first")
        ptr = iface["data"][0]
        if not ptr:
            raise ValueError(f"input {name}: the device array has no data (a null pointer)")
        strides = iface.get("strides")
        pitch = shape[1] * item
        if strides is not None:
            strides = tuple(int(s) for s in strides)
            if strides[1] != item and shape[1] > 1:
                raise ValueError(f"input {name}: the values of a row must be adjacent (inner stride {strides[1]}, item size {item}): "
                                 "call .contiguous() on the device first")
            if shape[0] > 1:
                pitch = strides[0]
            if pitch < shape[1] * item or pitch % item:
                raise ValueError(f"input {name}: row stride {pitch} must be a multiple of the item size {item} and at least a row "
                                 f"({shape[1] * item} bytes): call .contiguous() on the device first")
        if shape[1] != n:
            raise ValueError(f"Input size does not match program vector size (input {name}: rows of {shape[1]} values, vector size {n})")
        if B is None:
            B, first = shape[0], name
        elif shape[0] != B:
            raise ValueError(f"input {name} has {shape[0]} instances, {first} has {B}")
        out[name] = (int(ptr), code, shape[0], shape[1], int(pitch), _producer_stream(x, iface, stream))
    if B is not None and B < 1:
        raise ValueError(f"input {first} has no instances")
    return out, B, first


def _encrypt_array(self, arrays, signature, seed=0, plain_arrays=None, stream=None):
    """encrypt_batch(rows, signature, device_sampling=True, seed=seed) for arrays: `arrays` maps every
    encrypted input to an array [B, n] — uint8, float32 and float64 cross PCIe in their own type and are converted on
    the GPU — and every other input to the one value all instances share.  Returns a SEALValuationBatch whose instance b
    is encrypt_batch's instance b word for word; per name the instances stay in batched handles of at most 64.
    Raises without a HIP device, with EVA_DEVICE_CLIENT=0, with resident = False and for a value the device encoder
    cannot take: there is no host path behind this call.
    plain_arrays: {name: array [B, n]} for unencrypted (Raw) inputs that differ per instance, kept in
    their own type; execute_batch encodes a group's rows on the device where the program encodes the input.  They stay
    host arrays: a device array there is refused.
    Device arrays: an encrypted input may be any object with __cuda_array_interface__ — a torch tensor
    on the GPU, a pitched slice t[:, :n] of one, a DeviceArray of decrypt_array(device=True) — of shape [B, n] and uint8,
    float32 or float64.  Its rows are read in place on the key pair's GPU: no value byte crosses PCIe, one wait per
    such array (for the 8 bytes a row its encodability check brings back), and for one seed the batch equals the one its
    host copy gives, word for word.  stream: the stream the array was written on (an address or an object with
    .cuda_stream); None means the interface's own stream entry, else torch's current stream for a tensor's device, else
    that the caller has synchronised."""
    for name, x in (plain_arrays or {}).items():
        if is_device_array(x):
            raise ValueError(f"plain_arrays stays on the host: input {name} is a device array (pass its rows as a numpy array)")
    device = {name: x for name, x in arrays.items() if is_device_array(x)}
    if not device:
        enc, shared, B = normalise_arrays(arrays, signature)
        devs = {}
    else:
        # device arrays: the rows are read where they are, after everything `stream` holds so far (default:
        # the interface's own stream entry, else torch's current stream for a tensor's device); host and device arrays mix by name
        devs, B, first = normalise_device_arrays(device, signature, stream)
        host = {name: x for name, x in arrays.items() if name not in device}
        enc, shared, Bh = normalise_arrays(host, signature, allow_none=True)
        if Bh is not None and Bh != B:
            other = next(iter(enc))
            raise ValueError(f"input {other} has {Bh} instances, {first} has {B}")
    plains = normalise_plain_arrays(plain_arrays, signature, B)
    for name in plains:
        if name in shared:
            raise ValueError(f"input {name} is given twice: in arrays and in plain_arrays")
    if not devs:
        return self._encrypt_array(enc, shared, signature, seed, plains)
    return self._encrypt_array(enc, shared, signature, seed, plains, devs)


_SEALPublic.encrypt_array = _encrypt_array
_SEALSecret.encrypt_array = _encrypt_array
