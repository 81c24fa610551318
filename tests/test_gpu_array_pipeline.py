"""GPU: arrays in, batched handles through execute_batch, arrays out.  encrypt_array against
encrypt_batch(..., device_sampling=True) of the same seed word for word on both key kinds; the whole pipeline
decrypt_array(execute_batch(encrypt_array)) against the list path's ciphertext words and float64 bit patterns and against
the oracle's walk, with evah_ct_stack's counters standing still; the bytes that cross PCIe; and a SEALValuationBatch's
instances as ordinary valuations for execute, decrypt, save and load.  70 instances are two segments (64 + 6), and with
batch_chunk = 12 a group boundary (60 .. 72) would cross the segment boundary if groups were not cut there."""
import numpy as np
import pytest

from eva import EvaProgram, Input, Output, load, save
from eva.ckks import CKKSCompiler
from eva.seal import SEALValuationBatch, generate_keys
from evatest import oracle_execute
from test_gpu_client_batch import _bits_equal, _same

pytestmark = pytest.mark.gpu

VEC, N, SCALE_BITS = 8, 1024, 30


def _program():
    """a multiply, a rotation and two inputs"""
    prog = EvaProgram('arrayflow', vec_size=VEC)
    with prog:
        x, y = Input('x'), Input('y')
        Output('z', x * y + (x << 1))
        Output('w', x - y)
    prog.set_input_scales(SCALE_BITS)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    params.poly_modulus_degree = N
    return compiled, params, sig


def _second_program():
    """takes the outputs of _program as they are: no rescale, so the first program's parameters serve"""
    prog = EvaProgram('second', vec_size=VEC)
    with prog:
        z, w = Input('z'), Input('w')
        Output('z', z + z)
        Output('w', -w)
    prog.set_input_scales(SCALE_BITS)
    prog.set_output_ranges(20)
    return CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)[0]


@pytest.fixture(scope="module")
def flow():
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 6)
    return compiled, sig, pub, sec


def _arrays(B, dtype, seed=8):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return {n: rng.integers(0, 4, size=(B, VEC), dtype=np.uint8) for n in ('x', 'y')}
    return {n: rng.uniform(-2, 2, (B, VEC)).astype(dtype) for n in ('x', 'y')}


def _rows_as_lists(arrays):
    B = len(next(iter(arrays.values())))
    return [{n: [float(v) for v in a[b]] for n, a in arrays.items()} for b in range(B)]


# ---- 5. encrypt parity with the list path

@pytest.mark.parametrize("B", [5, 70])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32, np.float64], ids=["u8", "f32", "f64"])
def test_encrypt_array_equals_encrypt_batch_of_the_same_seed(flow, B, dtype):
    compiled, sig, pub, sec = flow
    arrays = _arrays(B, dtype)
    rows = _rows_as_lists(arrays)
    for ctx, want in ((pub, pub.encrypt_batch(rows, sig, device_sampling=True, seed=3)),
                      (sec, sec.encrypt_batch(rows, sig, seed=3, device_sampling=True))):
        vb = ctx.encrypt_array(arrays, sig, seed=3)
        assert isinstance(vb, SEALValuationBatch) and len(vb) == B and sorted(vb.names()) == ['x', 'y']
        assert vb.segments('x') == vb.segments('y') == ([64, 6] if B == 70 else [5])
        assert len(vb.to_list()) == B
        for b in range(B):
            one = vb[b]
            assert all(one.is_resident(n) for n in ('x', 'y'))
            _same(one, want[b])
            assert [one.seed(n) for n in ('x', 'y')] == [want[b].seed(n) for n in ('x', 'y')]
    assert vb[0].seed('x') is not None and pub.encrypt_array(arrays, sig, seed=3)[0].seed('x') is None
    _same(vb[-1], want[B - 1])
    with pytest.raises(IndexError):
        vb[B]


def test_encrypt_array_has_no_silent_fallback(flow, monkeypatch):
    compiled, sig, pub, sec = flow
    arrays = _arrays(3, np.float32)
    bad = {n: a.copy() for n, a in arrays.items()}
    bad['y'][2, 5] = np.inf
    for ctx in (pub, sec):
        with pytest.raises(RuntimeError, match="input y, instance 2: the device encoder cannot take these values"):
            ctx.encrypt_array(bad, sig)
    keep = pub.resident
    pub.resident = False
    try:
        with pytest.raises(RuntimeError, match="encrypt_array needs resident valuations"):
            pub.encrypt_array(arrays, sig)
    finally:
        pub.resident = keep
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")
    pub0, sec0 = generate_keys(_program()[1], 6)
    for ctx in (pub0, sec0):
        with pytest.raises(RuntimeError, match="EVA_DEVICE_CLIENT=0 keeps the client on the host"):
            ctx.encrypt_array(arrays, sig)


# ---- 6. end to end

@pytest.mark.parametrize("kind", ["public", "symmetric"])
def test_pipeline_equals_the_list_path_and_the_oracle_without_a_stack_copy(flow, kind):
    compiled, sig, pub, sec = flow
    B = 70
    arrays = _arrays(B, np.uint8 if kind == "public" else np.float32)
    rows = _rows_as_lists(arrays)
    ctx = pub if kind == "public" else sec
    keep = pub.batch_chunk
    pub.batch_chunk = 12   # groups of 12: 60 .. 72 would span the segments 0 .. 64 and 64 .. 70
    try:
        vb = ctx.encrypt_array(arrays, sig, seed=11)
        s0 = pub.stack_stats()
        outs = pub.execute_batch(compiled, vb)
        s1 = pub.stack_stats()
        assert s1 == s0, "the array path stacks nothing"
        assert isinstance(outs, SEALValuationBatch) and len(outs) == B and sorted(outs.names()) == ['w', 'z']
        assert outs.segments('z') == outs.segments('w') == [12, 12, 12, 12, 12, 4, 6]
        got = sec.decrypt_array(outs, sig)
        assert pub.stack_stats() == s1
        encs = (pub.encrypt_batch(rows, sig, device_sampling=True, seed=11) if kind == "public"
                else sec.encrypt_batch(rows, sig, seed=11, device_sampling=True))
        s2 = pub.stack_stats()
        louts = pub.execute_batch(compiled, encs)
        s3 = pub.stack_stats()
        assert s3["calls"] == s2["calls"] + 2 * 6 and s3["instances"] == s2["instances"] + 2 * B, "the list path stacks every input of every group"
        want = sec.decrypt_batch(louts, sig)
    finally:
        pub.batch_chunk = keep
    assert sorted(got) == ['w', 'z']
    for n in ('w', 'z'):
        assert got[n].shape == (B, VEC) and got[n].dtype == np.float64
        for b in range(B):
            assert _bits_equal(got[n][b], want[b][n]), f"output {n}, instance {b}"
    for b in range(B):
        _same(outs[b], louts[b])
    for b in (0, B - 1):   # the oracle's walk over the same input words
        _same(outs[b], oracle_execute(pub, compiled, vb[b]))
    # the doubles are those of the plain computation up to CKKS noise
    x, y = arrays['x'].astype(np.float64), arrays['y'].astype(np.float64)
    assert np.abs(got['z'] - (x * y + np.roll(x, -1, axis=1))).max() < 1e-2
    assert np.abs(got['w'] - (x - y)).max() < 1e-2
    # float32 out: the same doubles rounded to nearest-even, and a list of valuations is read as single handles
    f32 = sec.decrypt_array(outs, sig, dtype=np.float32)
    for n in ('w', 'z'):
        assert f32[n].dtype == np.float32 and np.array_equal(f32[n].view(np.uint32), got[n].astype(np.float32).view(np.uint32))
    from_list = sec.decrypt_array(louts[:9] + outs.to_list()[9:20], sig)
    for n in ('w', 'z'):
        assert np.array_equal(from_list[n].view(np.uint64), got[n][:20].view(np.uint64))


def test_multi_device_modes_go_through_the_list_path(flow):
    """devices / shard set: execute_batch on a batch is to_list(), the list path and its results as segments of one"""
    compiled, sig, pub, sec = flow
    arrays = _arrays(5, np.float32, seed=9)
    ref = pub.execute_batch(compiled, pub.encrypt_array(arrays, sig, seed=2))
    pub2, sec2 = generate_keys(_program()[1], 6, devices=[0, 256], shard="dag")   # same seed: same keys; two states of device 0
    pub2.batch_chunk = 2
    vb = pub2.encrypt_array(arrays, sig, seed=2)
    outs = pub2.execute_batch(compiled, vb)
    assert isinstance(outs, SEALValuationBatch) and len(outs) == 5 and outs.segments('z') == [1] * 5
    for b in range(5):
        _same(outs[b], ref[b])
    got, want = sec2.decrypt_array(outs, sig), sec.decrypt_array(ref, sig)
    for n in ('w', 'z'):
        assert np.array_equal(got[n].view(np.uint64), want[n].view(np.uint64))


# ---- 7. transfer bytes and interop

@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["u8", "f32"])
def test_the_array_crosses_pcie_in_its_own_type(flow, dtype):
    compiled, sig, pub, sec = flow
    B = 70
    arrays = _arrays(B, dtype)
    item = np.dtype(dtype).itemsize
    pub.encrypt_array(arrays, sig)   # keys and tables are on the device afterwards
    sec.encrypt_array(arrays, sig)
    for ctx, extra in ((pub, 0), (sec, 32 * B)):
        before = pub.transfer_stats()
        ctx.encrypt_array(arrays, sig)
        after = pub.transfer_stats()
        assert after["h2d_bytes"] - before["h2d_bytes"] == 2 * (B * VEC * item + 32 * B + extra)
        assert after["ct_uploads"] == before["ct_uploads"] and after["d2h_bytes"] == before["d2h_bytes"]


def test_batches_chain_and_their_instances_are_ordinary_valuations(flow, tmp_path):
    compiled, sig, pub, sec = flow
    second = _second_program()
    B = 9
    arrays = _arrays(B, np.uint8, seed=4)
    vb = sec.encrypt_array(arrays, sig, seed=5)
    s0 = pub.stack_stats()
    mid = pub.execute_batch(compiled, vb)
    last = pub.execute_batch(second, mid)   # the result of one program is the input of the next
    assert pub.stack_stats() == s0 and isinstance(last, SEALValuationBatch) and len(last) == B
    got = sec.decrypt_array(last, sig)
    x, y = arrays['x'].astype(np.float64), arrays['y'].astype(np.float64)
    assert np.abs(got['z'] - 2 * (x * y + np.roll(x, -1, axis=1))).max() < 1e-2
    assert np.abs(got['w'] + (x - y)).max() < 1e-2
    # the same two programs on the instances as a list
    lmid = pub.execute_batch(compiled, vb.to_list())
    llast = pub.execute_batch(second, lmid)
    for b in range(B):
        _same(mid[b], lmid[b])
        _same(last[b], llast[b])
    # one instance through the single calls
    one = vb[4]
    single = pub.execute(compiled, one)
    _same(single, mid[4])
    mid_arr = sec.decrypt_array(mid, sig)
    for n, v in sec.decrypt(mid[4], sig).items():
        assert _bits_equal(v, mid_arr[n][4]), n
    for n, v in sec.decrypt(one, sig).items():
        assert np.abs(np.array(v) - arrays[n][4]).max() < 1e-4
    # save / load: a symmetric value is still written seeded (c0 + seed), a public one whole
    path = str(tmp_path / "one.sealvals")
    save(one, path)
    back = load(path)
    for n in ('x', 'y'):
        assert back.seed(n) == one.seed(n) is not None and back.on_host(n) and not back.is_resident(n)
    _same(back, one)
    pone = pub.encrypt_array(arrays, sig, seed=5)[4]
    ppath = str(tmp_path / "pub.sealvals")
    save(pone, ppath)
    _same(load(ppath), pone)
    assert (tmp_path / "one.sealvals").stat().st_size <= 0.55 * (tmp_path / "pub.sealvals").stat().st_size
