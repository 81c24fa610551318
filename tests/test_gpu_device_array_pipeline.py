"""GPU: device arrays through the Python surface.  encrypt_array from rows in device memory against
encrypt_array from their numpy copy, word for word for one seed on both key kinds; execute_batch and
decrypt_array(device=True) against the host path bit for bit (uint8 by numpy's rule); host and device arrays mixed by name;
the refusals that name input and instance; two key pairs chained through device memory with the transfer counters
standing still for value bytes; torch tensors, pitched slices and side streams; and the zeroing of a dropped DeviceArray.
N = 4096 is the two-pass FFT; 70 instances are two segments (64 + 6)."""
import numpy as np
import pytest

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import DeviceArray, SEALValuationBatch, generate_keys
from eva_amd import backend
from eva_amd.hostref import coeff_modulus_create
from test_gpu_client_batch import _same

pytestmark = pytest.mark.gpu

VEC, SCALE_BITS = 64, 30


def _program(N, name='devflow'):
    prog = EvaProgram(name, vec_size=VEC)
    with prog:
        x, y = Input('x'), Input('y')
        Output('z', x * y + (x << 1))
        Output('w', x - y)
    prog.set_input_scales(SCALE_BITS)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    params.poly_modulus_degree = N
    return compiled, params, sig


@pytest.fixture(scope="module")
def flow():
    compiled, params, sig = _program(4096)
    pub, sec = generate_keys(params, 6)
    stage = backend.Context(1024, coeff_modulus_create(1024, [40, 40]))   # a queue of GPU 0 to stage test arrays through
    yield compiled, sig, pub, sec, stage
    stage.close()


def _arrays(B, dtype, seed=8):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return {n: rng.integers(0, 4, size=(B, VEC), dtype=np.uint8) for n in ('x', 'y')}
    return {n: rng.uniform(-2, 2, (B, VEC)).astype(dtype) for n in ('x', 'y')}


def _on_device(stage, a, pitch=None):
    """the rows of `a` in device memory of GPU 0, one row into a fresh buffer, optionally pitched"""
    B, n = a.shape
    pitch = n * a.itemsize if pitch is None else pitch
    img = np.full(((1 + B) * pitch + 7) // 8 * 8, 0xA5, dtype=np.uint8)
    for b in range(B):
        img[(1 + b) * pitch:(1 + b) * pitch + n * a.itemsize] = a[b:b + 1].view(np.uint8).reshape(-1)
    buf = stage.buffer(img.size // 8)
    buf.upload_bytes(img)
    return buf.view((B, n), a.dtype, pitch, pitch)


def _same_batches(a, b):
    assert len(a) == len(b) and sorted(a.names()) == sorted(b.names())
    for n in a.names():
        assert a.segments(n) == b.segments(n)
    for i in range(len(a)):
        _same(a[i], b[i])
        assert [a[i].seed(n) for n in sorted(a.names())] == [b[i].seed(n) for n in sorted(b.names())]


def _u8_rule(d):
    return np.clip(np.rint(np.nan_to_num(d, nan=0.0)), 0, 255).astype(np.uint8)


# ---- 1. encrypt parity with the host copy

@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=["u8", "f32", "f64"])
def test_device_rows_encrypt_as_their_host_copy(flow, B, dtype):
    compiled, sig, pub, sec, stage = flow
    arrays = _arrays(B, dtype)
    item = np.dtype(dtype).itemsize
    for pitch in (None, (VEC + 3) * item):
        dev = {n: _on_device(stage, a, pitch) for n, a in arrays.items()}
        for ctx in (pub, sec):
            want = ctx.encrypt_array(arrays, sig, seed=3)
            got = ctx.encrypt_array(dev, sig, seed=3)
            assert isinstance(got, SEALValuationBatch) and got.segments('x') == ([64, 6] if B == 70 else [5])
            _same_batches(got, want)
            mixed = ctx.encrypt_array({'x': dev['x'], 'y': arrays['y']}, sig, seed=3)   # host and device arrays by name
            _same_batches(mixed, want)


def test_pipeline_on_device_equals_the_host_path(flow):
    compiled, sig, pub, sec, stage = flow
    B = 70
    arrays = _arrays(B, np.uint8)
    dev = {n: _on_device(stage, a, VEC + 1) for n, a in arrays.items()}
    outs = pub.execute_batch(compiled, sec.encrypt_array(dev, sig, seed=11))
    ref = pub.execute_batch(compiled, sec.encrypt_array(arrays, sig, seed=11))
    _same_batches(outs, ref)
    host = {dt: sec.decrypt_array(ref, sig, dtype=dt) for dt in (np.float64, np.float32)}
    for dt in (np.float64, np.float32, np.uint8):
        got = sec.decrypt_array(outs, sig, dtype=dt, device=True)
        assert sorted(got) == ['w', 'z']
        for n in ('w', 'z'):
            a = got[n]
            assert isinstance(a, DeviceArray) and a.shape == (B, VEC) and a.dtype == np.dtype(dt)
            cai = a.__cuda_array_interface__
            assert cai["version"] == 3 and cai["shape"] == (B, VEC) and cai["strides"] is None and cai["data"] == (a.ptr, False)
            assert cai["typestr"] == np.dtype(dt).str
            rows = a.to_numpy()
            assert rows.shape == (B, VEC) and rows.dtype == np.dtype(dt)
            if dt is np.uint8:
                assert np.array_equal(rows, _u8_rule(host[np.float64][n])), n
                assert np.array_equal(rows, sec.decrypt_array(outs, sig, dtype=np.uint8)[n]), n   # uint8 to the host: the same rule
            else:
                u = f"u{np.dtype(dt).itemsize}"
                assert np.array_equal(rows.view(u), host[dt][n].view(u)), n
    x, y = arrays['x'].astype(np.float64), arrays['y'].astype(np.float64)
    z = sec.decrypt_array(outs, sig, dtype=np.uint8, device=True)['z'].to_numpy()
    assert np.array_equal(z, _u8_rule(x * y + np.roll(x, -1, axis=1)))   # small integers: the noise is far from a tie


def test_a_refusal_names_input_and_instance(flow):
    compiled, sig, pub, sec, stage = flow
    arrays = _arrays(70, np.float32)
    for bad, b in ((np.inf, 66), (np.nan, 0), (2.0 ** 40, 69)):
        v = arrays['y'].copy()
        v[b, 5] = bad
        dev = {'x': _on_device(stage, arrays['x']), 'y': _on_device(stage, v, (VEC + 3) * 4)}
        for ctx in (pub, sec):
            with pytest.raises(RuntimeError, match=f"input y, instance {b}: the device encoder cannot take these values"):
                ctx.encrypt_array(dev, sig)
            with pytest.raises(RuntimeError, match=f"input y, instance {b}: the device encoder cannot take these values"):
                ctx.encrypt_array({'x': arrays['x'], 'y': v}, sig)   # the host rows: the same verdict
    dev = {n: _on_device(stage, a) for n, a in arrays.items()}
    with pytest.raises(ValueError, match="plain_arrays stays on the host: input x is a device array"):
        pub.encrypt_array({'y': dev['y']}, sig, plain_arrays={'x': dev['x']})
    host_rows = type("H", (), {"__cuda_array_interface__": {"shape": (70, VEC), "typestr": "<f4", "data": (arrays['x'].ctypes.data, False),
                                                           "version": 3, "strides": None}})()
    with pytest.raises(RuntimeError, match="values is host memory"):
        pub.encrypt_array({'x': host_rows, 'y': arrays['y']}, sig)
    pub.encrypt_array(dev, sig)   # the contexts go on


# ---- 2. two key pairs chained through device memory

def test_two_key_pairs_chain_without_a_value_byte_over_pcie(flow):
    compiled, sig, pub, sec, stage = flow
    compiled_b, params_b, sig_b = _program(2048, 'second')
    pub_b, sec_b = generate_keys(params_b, 9)
    B = 70
    arrays = _arrays(B, np.uint8, seed=4)
    outs = pub.execute_batch(compiled, sec.encrypt_array(arrays, sig, seed=5))
    for ctx in (pub_b, sec_b):
        ctx.encrypt_array(arrays, sig_b)   # keys and tables of pair B are on the device afterwards
    for dt in (np.uint8, np.float32):
        a0, b0 = pub.transfer_stats(), pub_b.transfer_stats()
        mid = sec.decrypt_array(outs, sig, dtype=dt, device=True)       # pair A's outputs stay in HBM ...
        vb = sec_b.encrypt_array({'x': mid['z'], 'y': mid['w']}, sig_b, seed=7)   # ... and are pair B's inputs
        a1, b1 = pub.transfer_stats(), pub_b.transfer_stats()
        assert a1 == a0, "decrypting into device memory moves nothing across PCIe"
        assert b1["h2d_bytes"] - b0["h2d_bytes"] == 2 * 64 * B, "two inputs: an error key and a seed per instance, no value bytes"
        assert b1["d2h_bytes"] - b0["d2h_bytes"] == 2 * 8 * B, "two inputs: the 8-byte sum of each row"
        assert b1["ct_uploads"] == b0["ct_uploads"] and b1["pt_uploads"] == b0["pt_uploads"]
        want = sec_b.encrypt_array({'x': mid['z'].to_numpy(), 'y': mid['w'].to_numpy()}, sig_b, seed=7)
        _same_batches(vb, want)
        pvb = pub_b.encrypt_array({'x': mid['z'], 'y': mid['w']}, sig_b, seed=7)
        _same_batches(pvb, pub_b.encrypt_array({'x': mid['z'].to_numpy(), 'y': mid['w'].to_numpy()}, sig_b, seed=7))
        if dt is np.uint8:
            last = sec_b.decrypt_array(pub_b.execute_batch(compiled_b, vb), sig_b)
            z, w = mid['z'].to_numpy().astype(np.float64), mid['w'].to_numpy().astype(np.float64)
            assert np.abs(last['z'] - (z * w + np.roll(z, -1, axis=1))).max() < 1e-1
            assert np.abs(last['w'] - (z - w)).max() < 1e-2


# ---- 3. the memory of a dropped DeviceArray

def test_a_dropped_device_array_returns_its_memory_zeroed(flow):
    compiled, sig, pub, sec, stage = flow
    B = 5
    outs = pub.execute_batch(compiled, sec.encrypt_array(_arrays(B, np.float64), sig, seed=2))
    got = sec.decrypt_array(outs, sig, device=True)
    assert np.abs(got['z'].to_numpy()).min() > 0
    ptrs = sorted(a.ptr for a in got.values())
    del got
    # the pool hands the freed blocks out again, unwritten: read them back
    again = [sec._device_array(B, VEC, np.float64) for _ in range(2)]
    assert sorted(a.ptr for a in again) == ptrs
    for a in again:
        assert not a.to_numpy().view(np.uint64).any()


# ---- 4. torch

def test_torch_tensors_slices_and_side_streams(flow):
    torch = pytest.importorskip("torch")
    compiled, sig, pub, sec, stage = flow
    B = 70
    for dtype in (np.uint8, np.float32):
        arrays = _arrays(B, dtype, seed=12)
        want = {id(ctx): ctx.encrypt_array(arrays, sig, seed=13) for ctx in (pub, sec)}
        # on torch's current stream, contiguous and as a pitched slice t[:, :n]
        whole = {n: torch.from_numpy(a).to("cuda") for n, a in arrays.items()}
        wide = {n: torch.cat([t, t[:, :3]], dim=1) for n, t in whole.items()}
        sliced = {n: t[:, :VEC] for n, t in wide.items()}
        assert not sliced['x'].is_contiguous() and sliced['x'].stride(0) == VEC + 3
        for ctx in (pub, sec):
            _same_batches(ctx.encrypt_array(whole, sig, seed=13), want[id(ctx)])
            _same_batches(ctx.encrypt_array(sliced, sig, seed=13), want[id(ctx)])
        if dtype is np.uint8:
            continue
        # filled on a side stream just before the call, no host synchronisation in between
        side = torch.cuda.Stream()
        for ctx in (pub, sec):
            with torch.cuda.stream(side):
                big = torch.zeros((B, VEC + 3), dtype=whole['x'].dtype, device="cuda")
                filled = {}
                for n, a in arrays.items():
                    t = torch.zeros_like(big)
                    for _ in range(8):   # (some work in front of the final values)
                        t += 1
                    t[:, :VEC] = whole[n]
                    filled[n] = t[:, :VEC]
                inside = ctx.encrypt_array(filled, sig, seed=13)               # stream=None: torch's current stream
            _same_batches(inside, want[id(ctx)])
            with torch.cuda.stream(side):
                again = {n: torch.zeros_like(big) for n in arrays}
                for n in arrays:
                    again[n][:, :VEC] = whole[n]
            explicit = ctx.encrypt_array({n: t[:, :VEC] for n, t in again.items()}, sig, seed=13, stream=side)
            for t in again.values():   # an overwrite on the producer stream right behind the call cannot overtake the read
                with torch.cuda.stream(side):
                    t.zero_()
            _same_batches(explicit, want[id(ctx)])
    # a device tensor of another type is refused with what to convert, not carried through the host
    with pytest.raises(ValueError, match="a device array must be uint8, float32 or float64"):
        pub.encrypt_array({n: t.to(torch.float16) for n, t in whole.items()}, sig)
    # the output is torch's to view without a copy
    outs = pub.execute_batch(compiled, want[id(sec)])
    for dt in (np.float32, np.uint8):
        got = sec.decrypt_array(outs, sig, dtype=dt, device=True)
        for n, a in got.items():
            t = torch.as_tensor(a, device="cuda")
            assert t.data_ptr() == a.ptr and tuple(t.shape) == (B, VEC)
            assert np.array_equal(t.cpu().numpy(), a.to_numpy())
