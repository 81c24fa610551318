"""GPU: the client calls on arrays and batched handles at the C ABI.  evah_encode_encrypt_array /
_symmetric_array on uint8, float32 and float64 arrays against evah_encode_encrypt_sampled_many / _symmetric_sampled_many
on the float64 image, word for word (which ties the typed scatter to the oracle through test_gpu_sampled.py and
test_gpu_client_batch.py; one float64 case goes to the oracle directly); their refusals with the existing calls'
messages; evah_ct_slice as a view; evah_decrypt_decode_handles against evah_decrypt_decode_many on the unstacked
instances as float64 BIT PATTERNS, against the oracle's doubles, and its float32 rows against numpy's rounding.
Shapes: N = 1024 is one FFT launch and half a sampler workgroup with 30/40/41-bit primes, N = 4096 the two-pass FFT with
20- and 60-bit primes; batch 8 / 9 are the two ways seeds travel, 64 the largest call; n_values 1 and 2 leave every
uint8 and float32 row after the first unaligned."""
import numpy as np
import pytest

from eva_amd import _eva, backend
from test_gpu_client_batch import CHAINS, SCALE, _bits_equal, _env_of, _err, _known_ct

pytestmark = pytest.mark.gpu

sampled_small = _eva._seal._sampled_small
DTYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}


@pytest.fixture(params=[CHAINS[0], CHAINS[2]], ids=lambda c: f"N{c[0]}")
def env(request):
    return _env_of(request.param)


def _keys(env, batch):
    return [env.rng.integers(0, 256, size=32, dtype=np.uint8).tobytes() for _ in range(batch)]


def _largest_f32(n_values, scale=SCALE):
    """the largest float32 v for which a row (v, 0, ..., 0) still passes check_encodable: its bound is
    2 v (slots / n) scale / N = v scale / n, every factor a power of two, and must stay below 2^62"""
    return np.nextafter(np.float32(2.0 ** 62 * n_values / scale), np.float32(0))


def _values(env, dtype, batch, n_values):
    if dtype == "u8":
        v = env.rng.integers(0, 256, size=(batch, n_values), dtype=np.uint8)
        v.flat[0], v.flat[-1] = 255, 0
        if v.size > 2:
            v.flat[1] = 0
            v.flat[-2] = 255
        return v
    v = env.rng.uniform(-4, 4, (batch, n_values)).astype(DTYPES[dtype])
    if dtype == "f32":
        # the last row: the largest encodable value beside zeros, a negative zero and a denormal where the row has room;
        # the first row of a longer batch carries the negative zero and the denormal among ordinary values
        v[-1] = 0
        v[-1, 0] = _largest_f32(n_values)
        for row in ([-1] if batch == 1 else [0, -1]):
            if n_values >= 3:
                v[row, 1], v[row, 2] = -0.0, 1e-40
        if batch > 1 and n_values < 3:
            v[0, 0] = -0.0
            v[min(1, batch - 2), n_values - 1] = 1e-40
    return v


# ---- 1. typed encrypt against the existing sampled calls

@pytest.mark.parametrize("batch", [1, 8, 9, 64])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_array_calls_equal_the_sampled_calls_on_the_float64_image(env, dtype, batch):
    g, N, k = env.g, env.N, env.k
    for l in sorted({1, k - 1}):
        for n_values in (1, 2, 8, N // 2):
            values = _values(env, dtype, batch, n_values)
            assert values.dtype == DTYPES[dtype] and values.flags["C_CONTIGUOUS"]
            image = values.astype(np.float64)
            rkeys, seeds = _keys(env, batch), _keys(env, batch)
            ct = g.encode_encrypt_array(values, l, SCALE, rkeys)
            assert ct.batch == batch and ct.info() == (2, l, SCALE)
            want = g.encode_encrypt_sampled_many(image, l, SCALE, rkeys)
            assert np.array_equal(ct.download(), want.download()), f"public, l={l}, n_values={n_values}"
            cs = g.encode_encrypt_symmetric_array(values, l, SCALE, rkeys, seeds)
            assert cs.batch == batch and cs.info() == (2, l, SCALE)
            ws = g.encode_encrypt_symmetric_sampled_many(image, l, SCALE, rkeys, seeds)
            assert np.array_equal(cs.download(), ws.download()), f"symmetric, l={l}, n_values={n_values}"


def test_float32_extremes_are_in_the_inputs(env):
    """what the parity test above feeds: -0.0, a denormal and the largest value check_encodable lets through"""
    for n_values in (1, 2, 8, env.N // 2):
        top = _largest_f32(n_values)
        one = np.zeros((1, n_values), dtype=np.float32)
        one[0, 0] = np.nextafter(top, np.float32(np.inf))
        assert _err(env.g.encode_encrypt_array, one, 1, SCALE, [bytes(32)]) == "encoded values are too large"
        one[0, 0] = top
        env.g.encode_encrypt_array(one, 1, SCALE, [bytes(32)])
    v = _values(env, "f32", 9, 8)
    assert np.signbit(v[0, 1]) and v[0, 1] == 0 and 0 < v[0, 2] < np.finfo(np.float32).tiny and v[-1, 0] == _largest_f32(8)


def test_a_float64_array_against_the_oracle_built_ciphertext(env):
    g, N, k = env.g, env.N, env.k
    l = k - 1
    values = env.rng.uniform(-4, 4, (3, 8))
    rkeys = _keys(env, 3)
    got = g.encode_encrypt_array(values, l, SCALE, rkeys).download()
    for b in (0, 2):
        small = np.array([sampled_small(rkeys[b], p, N) for p in (0, 1, 2)], dtype=np.int8)
        assert np.array_equal(got[b], env.oracle_encrypt(values[b], l, small)), f"instance {b}"


# ---- 2. refusals

def test_array_refusals_are_those_of_the_existing_calls(env):
    g, N, k = env.g, env.N, env.k
    l = k - 1
    keys = lambda b: [bytes(32)] * b
    for dtype in DTYPES.values():
        vals = lambda b, n=8: np.ones((b, n), dtype=dtype)
        f64 = lambda b, n=8: np.ones((b, n), dtype=np.float64)
        for b in (0, 65):
            assert _err(g.encode_encrypt_array, vals(b), l, SCALE, keys(b)) == _err(g.encode_encrypt_sampled_many, f64(b), l, SCALE, keys(b))
            assert (_err(g.encode_encrypt_symmetric_array, vals(b), l, SCALE, keys(b), keys(b))
                    == _err(g.encode_encrypt_symmetric_sampled_many, f64(b), l, SCALE, keys(b), keys(b)))
            assert "batch must be 1..64" in _err(g.encode_encrypt_array, vals(b), l, SCALE, keys(b))
        for limbs in (0, k):
            assert _err(g.encode_encrypt_array, vals(2), limbs, SCALE, keys(2)) == _err(g.encode_encrypt_sampled_many, f64(2), limbs, SCALE, keys(2))
            assert (_err(g.encode_encrypt_symmetric_array, vals(2), limbs, SCALE, keys(2), keys(2))
                    == _err(g.encode_encrypt_symmetric_sampled_many, f64(2), limbs, SCALE, keys(2), keys(2)))
        # a value count that does not divide the slots
        assert _err(g.encode_encrypt_array, vals(2, 3), l, SCALE, keys(2)) == _err(g.encode_encrypt_sampled_many, f64(2, 3), l, SCALE, keys(2))
        assert "value count must divide the slot count" in _err(g.encode_encrypt_symmetric_array, vals(2, 3), l, SCALE, keys(2), keys(2))
        # null pointers
        assert _err(g.encode_encrypt_array, vals(2), l, SCALE, None) == "randomness pointer is null"
        assert _err(g.encode_encrypt_symmetric_array, vals(2), l, SCALE, None, keys(2)) == "error polynomial and seed are required"
        assert _err(g.encode_encrypt_symmetric_array, vals(2), l, SCALE, keys(2), None) == "error polynomial and seed are required"
        # an unknown dtype: the new message
        for code in (3, -1, 64):
            assert "unknown value dtype" in _err(g.encode_encrypt_array, vals(2), l, SCALE, keys(2), code)
            assert "unknown value dtype" in _err(g.encode_encrypt_symmetric_array, vals(2), l, SCALE, keys(2), keys(2), code)
    # too-large values in each type, with the verdict and the message of the float64 image: uint8 can only reach the bound
    # through the scale (mean 255 at 2^55 is 2^62.99), the float types also through a value, an infinity or a NaN
    big = 2.0 ** 55
    u8 = np.full((2, 8), 255, dtype=np.uint8)
    u8[0] = 1   # instance 0 passes, instance 1 does not
    want = _err(g.encode_encrypt_sampled_many, u8.astype(np.float64), l, big, keys(2))
    assert want == "encoded values are too large"
    assert _err(g.encode_encrypt_array, u8, l, big, keys(2)) == want
    assert _err(g.encode_encrypt_symmetric_array, u8, l, big, keys(2), keys(2)) == want
    g.encode_encrypt_array(u8[:1], l, big, keys(1))   # (the instance that passes, alone)
    for dtype in (np.float32, np.float64):
        for bad in (np.inf, -np.inf, np.nan, 2.0 ** 62 * 8 / SCALE):
            v = np.zeros((2, 8), dtype=dtype)
            v[1, 5] = bad
            assert _err(g.encode_encrypt_sampled_many, v.astype(np.float64), l, SCALE, keys(2)) == want
            assert _err(g.encode_encrypt_array, v, l, SCALE, keys(2)) == want, (dtype, bad)
            assert _err(g.encode_encrypt_symmetric_array, v, l, SCALE, keys(2), keys(2)) == want, (dtype, bad)
    # a capturing context (one real call is captured around the refusals, so that the graph is an ordinary one)
    ct = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), SCALE)
    v = np.ones((2, 8), dtype=np.uint8)
    g.capture_begin()
    try:
        neg = g.negate(ct)
        cap = [_err(g.encode_encrypt_array, v, l, SCALE, keys(2)), _err(g.encode_encrypt_symmetric_array, v, l, SCALE, keys(2), keys(2)),
               _err(g.decrypt_decode_handles, [ct], 8)]
        existing = _err(g.encode_encrypt_sampled_many, v.astype(np.float64), l, SCALE, keys(2))
    finally:
        g.graph_free(g.capture_end())
    del neg
    assert cap == [existing] * 3 and "cannot be captured" in existing
    # missing keys
    bare = backend.Context(N, env.primes)
    try:
        ctb = bare.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), SCALE)
        assert _err(bare.encode_encrypt_array, v, l, SCALE, keys(2)) == "public key not present"
        assert _err(bare.encode_encrypt_symmetric_array, v, l, SCALE, keys(2), keys(2)) == "secret key not present"
        assert _err(bare.decrypt_decode_handles, [ctb], 8) == _err(bare.decrypt_decode_many, [ctb], 8) == "secret key not present"
    finally:
        bare.close()


# ---- 3. evah_ct_slice

def _rows(ct):
    """the download of a handle with the batch axis, also for a batch of one"""
    s, l, _ = ct.info()
    return ct.download().reshape(ct.batch, s, l, ct.ctx.N)


def test_slices_are_views_of_their_rows(env):
    g, N, k = env.g, env.N, env.k
    l, B = k - 1, 9
    data = np.stack([np.stack([env.rand_poly(l) for _ in range(2)]) for _ in range(B)])
    parent = g.upload_ct_batch(data, SCALE)
    for b0, n in ((0, B), (0, 1), (B - 1, 1), (3, 5)):
        s = parent.slice(b0, n)
        assert s.batch == n and s.info() == (2, l, SCALE)
        assert np.array_equal(_rows(s), data[b0:b0 + n]), (b0, n)
    inner = parent.slice(3, 5).slice(1, 2)   # a slice of a slice: instances 4 and 5
    assert np.array_equal(_rows(inner), data[4:6])
    assert np.array_equal(inner.unstack(1).download(), data[5])
    # a slice of a mod-switched batched view: the polynomial stride stays that of l limbs
    lower = g.mod_switch(parent)
    s = lower.slice(3, 5)
    assert s.batch == 5 and s.info() == (2, l - 1, SCALE)
    assert np.array_equal(_rows(s), data[3:8, :, :l - 1])
    assert np.array_equal(_rows(s.slice(4, 1)), data[7:8, :, :l - 1])
    # out of range
    for b0, n in ((0, 0), (0, B + 1), (B, 1), (5, 5), (2 ** 32 - 1, 2)):
        assert _err(parent.slice, b0, n) == "instance range out of range", (b0, n)
    # a slice outlives its freed parent
    keep = parent.slice(2, 3)
    parent.free()
    lower.free()
    assert np.array_equal(_rows(keep), data[2:5])
    assert np.array_equal(_rows(s), data[3:8, :, :l - 1])


def test_a_consumer_of_batched_handles_takes_slices_as_handles(env):
    """The evaluator's calls on slices == the same calls on evah_ct_stack'ed singles.  evah_multiply_relinearize_rescale_many
    itself takes single ciphertexts only (a stacked handle of several is refused as a slice of several is), so it gets
    slices and stacks of one instance; the calls that take batched handles — evah_multiply_relinearize_rescale and
    evah_multiply_rescale_relinearize_many, what the scheduler issues for a group — get slices of four."""
    N, k = env.N, env.k
    l, B = k - 1, 9
    g = backend.Context(N, env.primes)   # (a context of its own: the shared one holds no relinearization key)
    try:
        rk = np.stack([np.stack([env.rand_poly(k) for _ in range(2)]) for _ in range(l)])
        g.upload_relin_key(rk)
        da, db = (np.stack([np.stack([env.rand_poly(l) for _ in range(2)]) for _ in range(B)]) for _ in range(2))
        A, Bh = g.upload_ct_batch(da, SCALE), g.upload_ct_batch(db, SCALE)
        bits = int(env.primes[l - 1]).bit_length()
        stacked = lambda h, b0, n: g.stack([h.unstack(b) for b in range(b0, b0 + n)])
        before = g.stack_stats()
        got = [g.multiply_relinearize_rescale_many([A.slice(b, 1) for b in (2, 8)], [Bh.slice(b, 1) for b in (2, 8)], bits),
               [g.multiply_relinearize_rescale(A.slice(1, 4), Bh.slice(1, 4), bits)],
               g.multiply_rescale_relinearize_many([A.slice(0, 4), A.slice(4, 4)], [Bh.slice(0, 4), Bh.slice(4, 4)], bits)]
        assert g.stack_stats() == before   # slices copy nothing ...
        want = [g.multiply_relinearize_rescale_many([stacked(A, b, 1) for b in (2, 8)], [stacked(Bh, b, 1) for b in (2, 8)], bits),
                [g.multiply_relinearize_rescale(stacked(A, 1, 4), stacked(Bh, 1, 4), bits)],
                g.multiply_rescale_relinearize_many([stacked(A, 0, 4), stacked(A, 4, 4)], [stacked(Bh, 0, 4), stacked(Bh, 4, 4)], bits)]
        assert g.stack_stats() == (before[0] + 10, before[1] + 28)   # ... which is what the counters show
        assert "takes single ciphertexts" in _err(g.multiply_relinearize_rescale_many, [A.slice(0, 4)], [Bh.slice(0, 4)], bits)
        for xs, ys, n in zip(got, want, (1, 4, 4)):
            assert len(xs) == len(ys)
            for x, y in zip(xs, ys):
                assert x.batch == y.batch == n and x.info() == y.info()
                assert np.array_equal(x.download(), y.download())
        # a slice of a result is an ordinary handle as well
        assert np.array_equal(_rows(got[2][1].slice(1, 2)), want[2][1].download()[1:3])
    finally:
        g.close()


# ---- 4. evah_decrypt_decode_handles

def _mixed_handles(env, l):
    """64 instances as a single handle, a batched handle, a slice and an unstack view; the same instances unstacked"""
    g = env.g
    data = [np.stack([env.rand_poly(l) for _ in range(2)]) for _ in range(70)]
    data[1] = _known_ct(env, l, 2, SCALE)       # an encoded message among the random residues
    data[40] = _known_ct(env, l, 2, SCALE)
    single = g.upload_ct(data[0], SCALE)
    batched = g.upload_ct_batch(np.stack(data[1:33]), SCALE)          # 32 instances
    parent = g.upload_ct_batch(np.stack(data[33:70]), SCALE)          # 37, of which a slice of 30 and one view are used
    sl, view = parent.slice(5, 30), parent.unstack(36)
    handles = [single, batched, sl, view]
    flat = [single] + [batched.unstack(b) for b in range(32)] + [parent.unstack(5 + b) for b in range(30)] + [view]
    words = [data[0]] + data[1:33] + data[38:68] + [data[69]]
    assert sum(h.batch for h in handles) == len(flat) == len(words) == 64
    return handles, flat, words


@pytest.mark.parametrize("n_out", [1, 8, "all"])
def test_decrypt_decode_handles_equals_many_on_the_unstacked_views(env, n_out):
    g, o, N = env.g, env.o, env.N
    n_out = N // 2 if n_out == "all" else n_out
    for l in sorted({1, env.k - 1}):
        handles, flat, words = _mixed_handles(env, l)
        got = g.decrypt_decode_handles(handles, n_out)
        assert got.shape == (64, n_out) and got.dtype == np.float64
        want = g.decrypt_decode_many(flat, n_out)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"l={l}"
        for b in (0, 1, 33, 35, 63):   # the oracle's doubles: every kind of handle, both encoded messages (rows 1 and 35)
            assert _bits_equal(got[b], o.decode(o.decrypt(words[b], env.sk), SCALE)[:n_out]), f"oracle: row {b} (l={l})"
        f32 = g.decrypt_decode_handles(handles, n_out, dtype=np.float32)
        assert f32.shape == (64, n_out) and f32.dtype == np.float32
        assert np.array_equal(f32.view(np.uint32), got.astype(np.float32).view(np.uint32)), f"float32, l={l}"
        # a mod-switched batched view beside a slice of it
        if l > 1:
            lower = g.mod_switch(handles[1])
            pair = [lower, lower.slice(30, 2)]
            low = g.decrypt_decode_handles(pair, n_out)
            ref = g.decrypt_decode_many([lower.unstack(b) for b in range(32)] + [lower.unstack(30), lower.unstack(31)], n_out)
            assert np.array_equal(low.view(np.uint64), ref.view(np.uint64))


def test_decrypt_decode_handles_refusals(env):
    g, N, k = env.g, env.N, env.k
    l = k - 1
    ct = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), SCALE)
    b64 = g.upload_ct_batch(np.stack([np.stack([env.rand_poly(l) for _ in range(2)]) for _ in range(64)]), SCALE)
    assert g.decrypt_decode_handles([b64], 8).shape == (64, 8)
    assert "more than 64 instances" in _err(g.decrypt_decode_handles, [b64, ct], 8)
    assert "more than 64 instances" in _err(g.decrypt_decode_handles, [ct] * 65, 8)
    assert _err(g.decrypt_decode_handles, [], 8) == _err(g.decrypt_decode_many, [], 8)
    lower = g.mod_switch(b64.slice(0, 2))
    assert "ciphertext 2: limb count" in _err(g.decrypt_decode_handles, [ct, ct, lower], 8)
    assert _err(g.decrypt_decode_handles, [ct, ct, lower], 8) == _err(g.decrypt_decode_many, [ct, ct, lower.unstack(0)], 8)
    other_scale = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(2)]), 2.0 * SCALE)
    assert "ciphertext 1: scale" in _err(g.decrypt_decode_handles, [b64.slice(0, 3), other_scale], 8)
    three = g.upload_ct(np.stack([env.rand_poly(l) for _ in range(3)]), SCALE)
    assert "ciphertext 1: size" in _err(g.decrypt_decode_handles, [ct, three], 8)
    for code in (backend.U8, 3, -1):
        assert "unknown output dtype" in _err(g.decrypt_decode_handles, [ct], 8, np.float64, code)
    for n_out in (0, N):
        assert _err(g.decrypt_decode_handles, [ct], n_out) == _err(g.decrypt_decode_many, [ct], n_out)
