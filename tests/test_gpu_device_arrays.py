"""GPU: the array calls on device memory at the C ABI, device memory from backend.DeviceBuffer, no torch.
evah_encode_encrypt_array_dev / _symmetric_array_dev against evah_encode_encrypt_array / _symmetric_array on the same rows
brought to the host, word for word (existing code, tied to the oracle by test_gpu_client_array.py); evah_rows_abs_sum_dev
against numpy; evah_decrypt_decode_rows against evah_decrypt_decode_handles' bit patterns and numpy's uint8 rule; the
refusals, each before a launch; the transfer counters.
Shapes: N = 1024 is one FFT launch and half a sampler workgroup, N = 4096 the two-pass FFT; batch 9 sends seeds as a
device buffer, 64 is the largest call; n_values 1 and 2 leave uint8 and float32 rows unaligned; a pitch of
n_values + 3 items (uint8 also n_values + 1: rows at odd bytes) and a base one row into the buffer exercise the row
addressing; 0xA5 fills every byte that is not a value."""
import ctypes as C

import numpy as np
import pytest

from eva_amd import backend
from test_gpu_client_array import DTYPES, _keys, _largest_f32, _mixed_handles, _values
from test_gpu_client_batch import CHAINS, SCALE, _env_of, _err

pytestmark = pytest.mark.gpu

FILL = 0xA5


@pytest.fixture(params=[CHAINS[0], CHAINS[2]], ids=lambda c: f"N{c[0]}")
def env(request):
    return _env_of(request.param)


def _stage(g, values, pitch=None):
    """values [B, n] in a fresh device buffer, row b at byte (1 + b) * pitch (a base one row in): (view, host image)"""
    B, n = values.shape
    item = values.itemsize
    pitch = n * item if pitch is None else pitch
    total = (1 + B) * pitch
    img = np.full((total + 7) // 8 * 8, FILL, dtype=np.uint8)
    for b in range(B):
        img[(1 + b) * pitch:(1 + b) * pitch + n * item] = values[b:b + 1].view(np.uint8).reshape(-1)
    buf = g.buffer(img.size // 8)
    buf.upload_bytes(img)
    return buf.view((B, n), values.dtype, pitch, pitch), img


def _pitches(dtype, n_values):
    item = np.dtype(DTYPES[dtype]).itemsize
    return [None, (n_values + 3) * item] + ([n_values + 1] if dtype == "u8" else [])


class _HostRows:
    """host memory dressed as rows (for the refusals)"""

    def __init__(self, a):
        self.a, self.shape, self.dtype, self.pitch, self.ptr = a, a.shape, a.dtype, a.strides[0], a.ctypes.data


# ---- 1. encrypt

@pytest.mark.parametrize("batch", [1, 9, 64])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_dev_calls_equal_the_array_calls_on_the_same_rows(env, dtype, batch):
    g, N, k = env.g, env.N, env.k
    for l in sorted({1, k - 1}):
        for n_values in (1, 2, 8, N // 2):
            values = _values(env, dtype, batch, n_values)
            rkeys, seeds = _keys(env, batch), _keys(env, batch)
            want = g.encode_encrypt_array(values, l, SCALE, rkeys).download()
            wants = g.encode_encrypt_symmetric_array(values, l, SCALE, rkeys, seeds).download()
            for pitch in _pitches(dtype, n_values):
                at = f"l={l}, n_values={n_values}, pitch={pitch}"
                rows, _ = _stage(g, values, pitch)
                sums = g.rows_abs_sum_dev(rows)
                ct = g.encode_encrypt_array_dev(rows, l, SCALE, rkeys)                       # row_sums NULL: computed by the call
                assert ct.batch == batch and ct.info() == (2, l, SCALE)
                assert np.array_equal(ct.download(), want), f"public, {at}"
                ct = g.encode_encrypt_array_dev(rows, l, SCALE, rkeys, row_sums=sums)
                assert np.array_equal(ct.download(), want), f"public, sums given, {at}"
                cs = g.encode_encrypt_symmetric_array_dev(rows, l, SCALE, rkeys, seeds, row_sums=sums)
                assert cs.batch == batch and cs.info() == (2, l, SCALE)
                assert np.array_equal(cs.download(), wants), f"symmetric, sums given, {at}"
                cs = g.encode_encrypt_symmetric_array_dev(rows, l, SCALE, rkeys, seeds)
                assert np.array_equal(cs.download(), wants), f"symmetric, {at}"


def test_back_to_back_dev_calls_without_a_drain_keep_their_keys(env):
    """more calls in flight than the queue has key slots, nothing waited for in between: every handle still holds the
    words of its own keys"""
    g, l = env.g, env.k - 1
    values = _values(env, "u8", 9, 8)
    rows, _ = _stage(g, values, 11)
    sums = g.rows_abs_sum_dev(rows)
    keys = [(_keys(env, 9), _keys(env, 9)) for _ in range(12)]
    cts = [g.encode_encrypt_symmetric_array_dev(rows, l, SCALE, ek, sd, row_sums=sums) for ek, sd in keys]
    for ct, (ek, sd) in zip(cts, keys):
        assert np.array_equal(ct.download(), g.encode_encrypt_symmetric_array(values, l, SCALE, ek, sd).download())


# ---- 2. row sums

@pytest.mark.parametrize("dtype", list(DTYPES))
def test_row_sums_against_numpy(env, dtype):
    g, N = env.g, env.N
    for B in (1, 9, 300):   # rows is not limited to 64
        for n_values in (1, 2, 8, 300, N // 2):
            values = _values(env, dtype, B, n_values)
            want = np.abs(values.astype(np.float64)).sum(axis=1)
            for pitch in _pitches(dtype, n_values):
                got = g.rows_abs_sum_dev(_stage(g, values, pitch)[0])
                assert got.shape == (B,) and got.dtype == np.float64
                if dtype == "u8" or n_values == 1:
                    assert np.array_equal(got, want), (B, n_values, pitch)   # integer sums below 2^53, or one term: exact
                else:
                    # n terms in a tree against numpy's order: each differs from the exact sum by at most n ulps
                    assert np.allclose(got, want, rtol=2 * n_values * 2.0 ** -52, atol=0), (B, n_values, pitch)
                assert np.array_equal(got, g.rows_abs_sum_dev(_stage(g, values, pitch)[0]))   # the same on every run


def test_the_encodable_boundary_is_exact_for_one_value_and_near_for_rows(env):
    g, N, k = env.g, env.N, env.k
    l = k - 1
    top = _largest_f32(1)
    for v, ok in ((top, True), (np.nextafter(top, np.float32(np.inf)), False), (-top, True)):
        rows, _ = _stage(g, np.array([[0.0], [v]], dtype=np.float32))
        sums = g.rows_abs_sum_dev(rows)
        assert sums[1] == abs(np.float64(v))
        for given in (None, sums):
            if ok:
                assert np.array_equal(g.encode_encrypt_array_dev(rows, l, SCALE, [bytes(32)] * 2, row_sums=given).download(),
                                      g.encode_encrypt_array(rows.to_numpy(), l, SCALE, [bytes(32)] * 2).download())
            else:
                assert _err(g.encode_encrypt_array_dev, rows, l, SCALE, [bytes(32)] * 2, given) == "encoded values are too large"
                assert _err(g.encode_encrypt_array, rows.to_numpy(), l, SCALE, [bytes(32)] * 2) == "encoded values are too large"
    # longer rows a factor of two and more from 2^62 on either side (bound = sum * scale / n): the tree and the host's
    # serial sum may differ in the last bits, and only there
    for dtype in (np.float32, np.float64):
        for n_values in (8, N // 2):
            inside = (env.rng.uniform(0.5, 1.0, (3, n_values)) * 2.0 ** 61 / SCALE).astype(dtype)
            inside[1] = -inside[1]
            rows, _ = _stage(g, inside, (n_values + 3) * inside.itemsize)
            got = g.encode_encrypt_array_dev(rows, l, SCALE, [bytes(32)] * 3)
            assert np.array_equal(got.download(), g.encode_encrypt_array(inside, l, SCALE, [bytes(32)] * 3).download())
            outside = inside.copy()
            outside[2] *= 8
            rows, _ = _stage(g, outside)
            assert _err(g.encode_encrypt_array_dev, rows, l, SCALE, [bytes(32)] * 3) == "encoded values are too large"
            assert _err(g.encode_encrypt_symmetric_array_dev, rows, l, SCALE, [bytes(32)] * 3, [bytes(32)] * 3) == "encoded values are too large"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_non_finite_rows_are_refused_and_the_context_goes_on(env, dtype):
    g, N, k = env.g, env.N, env.k
    l, B, n_values = k - 1, 64, 8
    lib = backend._lib
    good = env.rng.uniform(-4, 4, (B, n_values)).astype(dtype)
    for bad in (np.nan, np.inf, -np.inf):
        for where in ((0, 0), (0, n_values - 1), (B - 1, n_values // 2)):   # first element, last element, the last row only
            v = good.copy()
            v[where] = bad
            for pitch in (None, (n_values + 3) * v.itemsize):
                rows, _ = _stage(g, v, pitch)
                sums = g.rows_abs_sum_dev(rows)
                assert not np.isfinite(sums[where[0]]) and np.isfinite(np.delete(sums, where[0])).all()
                keys = backend._keys32([bytes(32)] * B, B)
                for given in (None, sums):
                    h = C.c_void_p()
                    sp = None if given is None else given.ctypes.data_as(C.POINTER(C.c_double))
                    rc = lib.evah_encode_encrypt_array_dev(g.h, B, C.c_void_p(rows.ptr), backend._DTYPES[np.dtype(dtype)], rows.pitch, None, sp,
                                                           n_values, l, SCALE, keys, C.byref(h))
                    assert rc != 0 and lib.evah_last_error().decode() == "encoded values are too large" and h.value is None
                    rc = lib.evah_encode_encrypt_symmetric_array_dev(g.h, B, C.c_void_p(rows.ptr), backend._DTYPES[np.dtype(dtype)], rows.pitch,
                                                                     None, sp, n_values, l, SCALE, keys, keys, C.byref(h))
                    assert rc != 0 and lib.evah_last_error().decode() == "encoded values are too large" and h.value is None
    rows, _ = _stage(g, good)
    rkeys = _keys(env, B)
    assert np.array_equal(g.encode_encrypt_array_dev(rows, l, SCALE, rkeys).download(), g.encode_encrypt_array(good, l, SCALE, rkeys).download())


# ---- 3. decrypt

def _dest(g, B, n_out, dtype, pitch):
    """a device destination [B, n_out] filled with 0xA5, rows pitched and one row into the buffer"""
    return _stage(g, np.full((B, n_out * np.dtype(dtype).itemsize), FILL, dtype=np.uint8).view(dtype), pitch)


def _u8_rule(d):
    return np.clip(np.rint(np.nan_to_num(d, nan=0.0)), 0, 255).astype(np.uint8)


def _gaps_untouched(view, img):
    """every byte of the buffer outside the rows still holds the fill pattern"""
    raw = view.buf.download_bytes()
    mask = np.ones(raw.size, dtype=bool)
    B, n = view.shape
    for b in range(B):
        mask[view.offset + b * view.pitch: view.offset + b * view.pitch + n * view.dtype.itemsize] = False
    return np.array_equal(raw[mask], img[mask]) and (img[mask] == FILL).all()


@pytest.mark.parametrize("n_out", [1, 8, "all"])
def test_decrypt_decode_rows_equals_handles(env, n_out):
    g, N = env.g, env.N
    n_out = N // 2 if n_out == "all" else n_out
    for l in sorted({1, env.k - 1}):
        handles, _, _ = _mixed_handles(env, l)
        lists = [handles]
        if l > 1:
            lower = g.mod_switch(handles[1])
            lists.append([lower, lower.slice(30, 2)])   # a mod-switched batched view beside a slice of it
        for hs in lists:
            B = sum(h.batch for h in hs)
            f64 = g.decrypt_decode_handles(hs, n_out)
            f32 = g.decrypt_decode_handles(hs, n_out, dtype=np.float32)
            for dtype, want in ((np.float64, f64), (np.float32, f32), (np.uint8, _u8_rule(f64))):
                item = np.dtype(dtype).itemsize
                for pitch in (None, (n_out + 3) * item) + ((n_out + 1,) if dtype is np.uint8 else ()):
                    at = f"l={l}, {np.dtype(dtype).name}, pitch={pitch}"
                    view, img = _dest(g, B, n_out, dtype, pitch)
                    g.decrypt_decode_rows(hs, n_out, view)
                    assert np.array_equal(view.to_numpy().view(f"u{item}"), want.view(f"u{item}")), at
                    assert _gaps_untouched(view, img), at
            # wait = 0, then the consumer's queue waits for this one (evah_ctx_wait) before it reads
            view, img = _dest(g, B, n_out, np.float64, (n_out + 3) * 8)
            g.decrypt_decode_rows(hs, n_out, view, wait=False)
            other = g.fork()
            other.wait_for(g)
            other.sync()
            assert np.array_equal(view.to_numpy().view(np.uint64), f64.view(np.uint64)) and _gaps_untouched(view, img)
            other.close()
            # host destinations: uint8, and rows with a pitch
            u8 = g.decrypt_decode_rows(hs, n_out, np.full((B, n_out), FILL, dtype=np.uint8))
            assert np.array_equal(u8, _u8_rule(f64))
            for dtype, want in ((np.float64, f64), (np.float32, f32), (np.uint8, _u8_rule(f64))):
                wide = np.frombuffer(bytes([FILL]) * (B * (n_out + 3) * np.dtype(dtype).itemsize), dtype=dtype).reshape(B, n_out + 3).copy()
                g.decrypt_decode_rows(hs, n_out, wide[:, :n_out])
                assert np.array_equal(wide[:, :n_out].view(f"u{wide.itemsize}"), want.view(f"u{wide.itemsize}"))
                assert (wide[:, n_out:].view(np.uint8) == FILL).all()


def test_uint8_rounding_where_it_can_go_wrong(env):
    """plaintexts encoding ties, the clamp's two ends, a negative and values far outside, as known ciphertexts"""
    g, o, N, k = env.g, env.o, env.N, env.k
    l = k - 1
    hard = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.4, -3, 300, 1e9, 0, 255, 128, 127.5, 1, 2, 3.5])
    m = o.encode(l, np.tile(hard, (N // 2) // hard.size), SCALE)
    cts = []
    for _ in range(3):
        ct = np.stack([env.rand_poly(l) for _ in range(2)])
        other = ct.copy()
        other[0] = 0
        rest = o.decrypt(other, env.sk)
        ct[0] = np.stack([(m[i].astype(object) - rest[i].astype(object)) % env.primes[i] for i in range(l)]).astype(np.uint64)
        cts.append(ct)
    h = g.upload_ct_batch(np.stack(cts), SCALE)
    f64 = g.decrypt_decode_handles([h], hard.size)
    assert np.allclose(f64, hard, rtol=1e-6, atol=1e-3)   # (the message is the one meant)
    view, _ = _dest(g, 3, hard.size, np.uint8, hard.size + 1)
    g.decrypt_decode_rows([h], hard.size, view)
    got = view.to_numpy()
    assert np.array_equal(got, _u8_rule(f64))
    assert np.array_equal(g.decrypt_decode_rows([h], hard.size, np.zeros((3, hard.size), dtype=np.uint8)), got)
    assert (got == 0).any() and (got == 255).any() and ((got > 0) & (got < 255)).any()   # not all-zero output
    assert got[0, 7] == 255 and got[0, 8] == 255 and got[0, 6] == 0 and got[0, 11] == 128
    # the rule itself on the values the decode cannot hit exactly: what the kernel computes for ties, NaN and infinities
    # is numpy's rule by construction of the comparison above; the ties are pinned through exactly representable doubles
    exact = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -0.5])
    assert np.array_equal(_u8_rule(exact), [0, 2, 2, 254, 255, 0])


# ---- 4. refusals, each before anything is launched

def test_dev_refusals(env):
    g, N, k = env.g, env.N, env.k
    l = k - 1
    keys = lambda b: [bytes(32)] * b
    values = np.ones((2, 8), dtype=np.float32)
    rows, _ = _stage(g, values, 44)
    ct = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), SCALE)
    dst, _ = _dest(g, 1, 8, np.float32, 44)
    enc = lambda *a, **kw: g.encode_encrypt_array_dev(*a, **kw)
    sym = lambda r, *a, **kw: g.encode_encrypt_symmetric_array_dev(r, l, SCALE, keys(r.shape[0]), keys(r.shape[0]), *a, **kw)

    def err(call, *a, **kw):
        with pytest.raises(RuntimeError) as e:
            call(*a, **kw)
        return str(e.value)

    # a host pointer, by name
    host = _HostRows(values)
    for message in (err(g.rows_abs_sum_dev, host), err(enc, host, l, SCALE, keys(2)), err(sym, host)):
        assert message.startswith("values is host memory")
    assert err(g.decrypt_decode_rows, [ct], 8, _HostRows(np.zeros((1, 8), dtype=np.float32))).startswith("out is host memory")
    # a short pitch, and one that is no multiple of the item size
    for call, args in ((g.rows_abs_sum_dev, (rows,)), (enc, (rows, l, SCALE, keys(2))), (sym, (rows,))):
        assert err(call, *args, pitch=28) == "row pitch is smaller than a row"
        assert err(call, *args, pitch=42) == "row pitch is not a multiple of the item size"
    assert err(g.decrypt_decode_rows, [ct], 8, dst, pitch=28) == "row pitch is smaller than a row"
    assert err(g.decrypt_decode_rows, [ct], 8, dst, pitch=42) == "row pitch is not a multiple of the item size"
    assert err(g.decrypt_decode_rows, [ct], 8, np.zeros((1, 8), dtype=np.float32), pitch=16) == "row pitch is smaller than a row"
    # an unknown dtype, in and out
    for code in (3, -1, 64):
        assert "unknown value dtype" in err(g.rows_abs_sum_dev, rows, dtype_code=code)
        assert "unknown value dtype" in err(enc, rows, l, SCALE, keys(2), dtype_code=code)
        assert "unknown value dtype" in err(sym, rows, dtype_code=code)
        assert "unknown output dtype" in err(g.decrypt_decode_rows, [ct], 8, dst, dtype_code=code)
    # 65 instances, and the other checks of the array calls with their messages
    many, _ = _stage(g, np.ones((65, 8), dtype=np.uint8))
    assert err(enc, many, l, SCALE, keys(65)) == err(g.encode_encrypt_array, np.ones((65, 8), dtype=np.uint8), l, SCALE, keys(65))
    assert "batch must be 1..64" in err(sym, many)
    assert err(enc, rows, k, SCALE, keys(2)) == err(g.encode_encrypt_array, values, k, SCALE, keys(2))
    three, _ = _stage(g, np.ones((2, 3), dtype=np.float32))
    assert err(enc, three, l, SCALE, keys(2)) == "value count must divide the slot count"
    assert err(enc, rows, l, SCALE, None) == "randomness pointer is null"
    assert err(g.encode_encrypt_symmetric_array_dev, rows, l, SCALE, keys(2), None) == "error polynomial and seed are required"
    # a capturing context (one real call is captured around the refusals, so that the graph is an ordinary one)
    g.capture_begin()
    try:
        neg = g.negate(ct)
        cap = [err(g.rows_abs_sum_dev, rows), err(enc, rows, l, SCALE, keys(2)), err(sym, rows), err(g.decrypt_decode_rows, [ct], 8, dst)]
        existing = err(g.encode_encrypt_array, values, l, SCALE, keys(2))
    finally:
        g.graph_free(g.capture_end())
    del neg
    assert cap == [existing] * 4 and "cannot be captured" in existing
    # the _handles messages for mixed limbs, scale and size: identical strings
    b3 = g.upload_ct_batch(np.stack([np.stack([env.rand_poly(l) for _ in range(2)]) for _ in range(3)]), SCALE)
    lower = g.mod_switch(b3.slice(0, 2))
    other_scale = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), 2.0 * SCALE)
    size3 = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(3)]), SCALE)
    big, _ = _dest(g, 66, 8, np.float32, None)
    for hs in ([ct, ct, lower], [b3, other_scale], [ct, size3], [], [ct] * 65):
        assert err(g.decrypt_decode_rows, hs, 8, big) == err(g.decrypt_decode_handles, hs, 8)
    for n_out in (0, N):
        assert err(g.decrypt_decode_rows, [ct], n_out, big, pitch=4 * N) == err(g.decrypt_decode_handles, [ct], n_out)
    # missing keys
    bare = backend.Context(N, env.primes)
    try:
        r2, _ = _stage(bare, values)
        assert err(bare.encode_encrypt_array_dev, r2, l, SCALE, keys(2)) == "public key not present"
        assert err(bare.encode_encrypt_symmetric_array_dev, r2, l, SCALE, keys(2), keys(2)) == "secret key not present"
    finally:
        bare.close()
    # nothing above disturbed the context
    assert np.array_equal(enc(rows, l, SCALE, keys(2)).download(), g.encode_encrypt_array(values, l, SCALE, keys(2)).download())


@pytest.mark.skipif(backend.device_count() < 2, reason="needs two GPUs")
def test_memory_of_another_gpu_is_refused(env):
    other = backend.Context(env.N, env.primes, device=1)
    try:
        rows, _ = _stage(other, np.ones((2, 8), dtype=np.float32))
        assert "is memory of GPU 1, this context runs on GPU 0" in _err(env.g.rows_abs_sum_dev, rows)
        assert "is memory of GPU 1, this context runs on GPU 0" in _err(env.g.encode_encrypt_array_dev, rows, env.k - 1, SCALE, [bytes(32)] * 2)
    finally:
        other.close()


# ---- 5. transfer counters

def test_a_dev_encryption_sends_keys_and_no_value_bytes(env):
    g, l = env.g, env.k - 1
    for B, n_values in ((9, 8), (64, env.N // 2)):
        values = _values(env, "f64", B, n_values)
        rows, _ = _stage(g, values)
        sums = g.rows_abs_sum_dev(rows)
        before = g.transfer_stats()
        g.encode_encrypt_array_dev(rows, l, SCALE, _keys(env, B), row_sums=sums)
        mid = g.transfer_stats()
        g.encode_encrypt_symmetric_array_dev(rows, l, SCALE, _keys(env, B), _keys(env, B), row_sums=sums)
        after = g.transfer_stats()
        assert mid[4] - before[4] == 32 * B and after[4] - mid[4] == 64 * B
        assert after[5] == before[5] and after[:4] == before[:4]
        g.encode_encrypt_array_dev(rows, l, SCALE, _keys(env, B))   # the sums computed by the call: 8 bytes a row come back
        assert g.transfer_stats()[5] - after[5] == 8 * B
        # the host-array call on the same rows, for the contrast
        h0 = g.transfer_stats()[4]
        g.encode_encrypt_array(values, l, SCALE, _keys(env, B))
        assert g.transfer_stats()[4] - h0 == 32 * B + values.nbytes
        # device rows out: nothing comes down; host rows count what they bring
        ct = g.encode_encrypt_array_dev(rows, l, SCALE, _keys(env, B), row_sums=sums)
        dst, _ = _dest(g, B, n_values, np.uint8, None)
        d0 = g.transfer_stats()[5]
        g.decrypt_decode_rows([ct], n_values, dst)
        assert g.transfer_stats()[5] == d0
        g.decrypt_decode_rows([ct], n_values, np.zeros((B, n_values), dtype=np.uint8))
        assert g.transfer_stats()[5] - d0 == B * n_values
