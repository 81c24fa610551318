"""GPU: plaintexts that differ per instance.  evah_pt_encode_array against evah_pt_encode of every row
and the oracle's encoder, word for word; add_plain / sub_plain / multiply_plain / weighted_sum / evah_elementwise_program /
evah_execute with a batched plaintext against the same call on every instance (evah_ct_slice + the single plaintext of
the row) and against the oracle; the refusals; and the product flow: execute_batch with an unencrypted input that differs
per instance, on lists and through encrypt_array(..., plain_arrays=...), against the oracle's walk and the single
execute() of each instance.
Shapes: N = 1024 is one FFT launch, N = 4096 two; batch 1 / 5 / 64; limbs 1 and k - 1; the interpreter's two shapes are
N = 1024 x B = 3 (one coefficient per thread) and N = 8192 x 2 limbs x B = 64 = 2^20 coefficients (two); 5 instances in
groups of 2 are ragged and reuse every queue, 70 are two segments."""
import ctypes as C

import numpy as np
import pytest

from eva import EvaProgram, Input, Output, evaluate
from eva.ckks import CKKSCompiler
from eva.metric import valuation_mse
from eva.seal import SEALValuationBatch, generate_keys
from eva_amd import backend
from evatest import oracle_execute
from oracle import pyoracle as po
import oplist as ol
from test_gpu_client_batch import CHAINS, SCALE, _bits_equal, _env_of, _err, _same

pytestmark = pytest.mark.gpu

DTYPES = {"u8": np.uint8, "f32": np.float32, "f64": np.float64}


@pytest.fixture(params=[CHAINS[0], CHAINS[2]], ids=lambda c: f"N{c[0]}")
def env(request):
    return _env_of(request.param)


@pytest.fixture
def env1k():
    return _env_of(CHAINS[0])


def _rows(env, dtype, batch, n_values, scale=SCALE):
    """rows of `dtype` with the edges among them where the batch has room: an all-zero row, a row of equal values, and
    (float types) a row at + and one at - the largest magnitude check_encodable lets through"""
    if dtype == "u8":
        v = env.rng.integers(0, 256, size=(batch, n_values), dtype=np.uint8)
        if batch >= 5:
            v[1], v[2] = 0, 255
        return v
    v = env.rng.uniform(-4, 4, (batch, n_values)).astype(DTYPES[dtype])
    if batch >= 5:
        top = DTYPES[dtype](2.0 ** 62 * n_values / scale)
        top = np.nextafter(top, DTYPES[dtype](0))
        v[1], v[2] = 0, 1.5
        v[3], v[4] = 0, 0
        v[3, 0], v[4, n_values - 1] = top, -top
    return v


def _ct_words(env, prefix, l):
    return np.stack([env.rng.integers(0, env.primes[i], size=tuple(prefix) + (env.N,), dtype=np.uint64) for i in range(l)], axis=len(prefix))


# ---- 1. the encoder

@pytest.mark.parametrize("batch", [1, 5, 64])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_encode_array_equals_the_single_encoder_and_the_oracle(env, dtype, batch):
    g, o, N, k = env.g, env.o, env.N, env.k
    for l in sorted({1, k - 1}):
        for n_values in (1, 8, N // 2):
            values = _rows(env, dtype, batch, n_values)
            image = values.astype(np.float64)
            pt = g.encode_pt_array(values, l, SCALE)
            assert pt.batch == batch and pt.info() == (l, SCALE)
            got = pt.download_instances()
            assert got.shape == (batch, l, N)
            for b in range(batch):
                assert np.array_equal(got[b], g.encode_pt(image[b], l, SCALE).download()), f"instance {b} (l={l}, n_values={n_values})"
            # the oracle applies SEAL's total-modulus rule, which the device encoder leaves to its callers: the rows at the
            # largest magnitude (coefficients up to 2^62) go to it only at a level whose modulus holds them
            fits = sum(int(q).bit_length() for q in env.primes[:l]) > 64
            for b in sorted({0, batch // 2, batch - 1} | (set(range(5)) if batch >= 5 and N == 1024 else set())):
                if dtype != "u8" and batch >= 5 and b in (3, 4) and not fits:
                    continue
                want = o.encode(l, np.tile(image[b], (N // 2) // n_values), SCALE)
                assert np.array_equal(got[b], want), f"oracle, instance {b} (l={l}, n_values={n_values})"
            # the stream-ordered form: the same words once the queue has been synchronised
            lazy = g.encode_pt_array(values, l, SCALE, wait=False)
            g.sync()
            assert np.array_equal(lazy.download_instances(), got)


def test_encode_array_counts_its_bytes_in_their_own_type(env1k):
    g = env1k.g
    for dtype, item in (("u8", 1), ("f32", 4), ("f64", 8)):
        v = _rows(env1k, dtype, 5, 8)
        before = g.transfer_stats()
        g.encode_pt_array(v, 2, SCALE)
        after = g.transfer_stats()
        assert after[4] - before[4] == 5 * 8 * item and after[5] == before[5] and after[:4] == before[:4]


def test_encode_array_refusals(env1k):
    g, N, k = env1k.g, env1k.N, env1k.k
    lib = backend.load()
    l = k - 1

    def raw(batch, values, dtype, n_values, limbs, scale, out=True, fn="evah_pt_encode_array"):
        h = C.c_void_p()
        rc = getattr(lib, fn)(g.h, batch, values.ctypes.data_as(C.c_void_p) if values is not None else None, dtype, n_values, limbs,
                              float(scale), C.byref(h) if out else None)
        assert rc != 0 and not h.value
        return lib.evah_last_error().decode()

    v = np.ones((65, 8))
    for fn in ("evah_pt_encode_array", "evah_pt_encode_array_async"):
        for b in (0, 65):
            assert raw(b, v, backend.F64, 8, l, SCALE, fn=fn) == "batch must be 1..64"
        assert raw(2, None, backend.F64, 8, l, SCALE, fn=fn) == "value pointer is null"
        assert raw(2, v, backend.F64, 8, l, SCALE, out=False, fn=fn) == "output pointer is null"
        for code in (3, -1, 64):
            assert "unknown value dtype" in raw(2, v, code, 8, l, SCALE, fn=fn)
        assert raw(2, v, backend.F64, 3, l, SCALE, fn=fn) == "value count must divide the slot count"
        for limbs in (0, k):
            assert raw(2, v, backend.F64, 8, limbs, SCALE, fn=fn) == "invalid limb count for this context"
    # a row that is too large, in each type, with the message of the single encoder
    for bad in (np.inf, np.nan, 2.0 ** 62 * 8 / SCALE):
        for dtype in (np.float32, np.float64):
            x = np.zeros((3, 8), dtype=dtype)
            x[2, 5] = bad
            assert _err(g.encode_pt_array, x, l, SCALE) == "encoded values are too large"
            assert _err(g.encode_pt, x[2].astype(np.float64), l, SCALE) == "encoded values are too large"
    u8 = np.full((2, 8), 255, dtype=np.uint8)
    u8[0] = 1
    assert _err(g.encode_pt_array, u8, l, 2.0 ** 55) == "encoded values are too large"
    g.encode_pt_array(u8[:1], l, 2.0 ** 55)
    # a capturing context (one real launch inside, so that the capture is not empty)
    ct = g.upload_ct(_ct_words(env1k, (2,), l), SCALE)
    g.capture_begin()
    try:
        for wait in (True, False):
            assert "cannot be captured into a graph" in _err(g.encode_pt_array, np.ones((2, 8)), l, SCALE, wait)
        neg = g.negate(ct)
    finally:
        g.graph_free(g.capture_end())
    del neg


def test_what_takes_one_plaintext_refuses_a_batch_of_them(env1k):
    g, N, k = env1k.g, env1k.N, env1k.k
    l = k - 1
    pb = g.encode_pt_array(env1k.rng.uniform(-1, 1, (3, 8)), l, SCALE)
    assert "takes a single plaintext" in _err(g.encrypt, pb, env1k.small(1)[0])
    assert "takes a single plaintext" in _err(g.encrypt_symmetric, pb, np.zeros(N, dtype=np.int8), bytes(32))
    assert "takes a single plaintext" in _err(pb.write, np.zeros((l, N), dtype=np.uint64))
    assert "takes a single plaintext" in _err(pb.download)
    ct = g.upload_ct(_ct_words(env1k, (2,), l), 2.0 ** 5)
    assert "multiply_plain_many takes single plaintexts" in _err(g.multiply_plain_many, [ct, ct], [pb, pb])
    ctb = g.upload_ct_batch(_ct_words(env1k, (3, 2), l), 2.0 ** 5)
    assert "rotate_weighted_sums takes weights that all instances share" in _err(g.rotate_weighted_sums, [([(ctb, 1), (ctb, 0)], [[pb, None]])])
    # a copy keeps the instances
    cp = backend.Plaintext(g, None)
    h = C.c_void_p()
    assert backend.load().evah_pt_copy(g.h, pb.h, C.byref(h)) == 0
    cp.h = h
    assert cp.batch == 3 and np.array_equal(cp.download_instances(), pb.download_instances())


# ---- 2. add_plain / sub_plain / multiply_plain

@pytest.mark.parametrize("form", ["size2", "size3", "mod_switched", "slice"])
def test_plain_ops_pair_instance_b_with_plaintext_b(env, form):
    g, o, N, k = env.g, env.o, env.N, env.k
    l, B = k - 1, 3
    size = 3 if form == "size3" else 2
    cs, ps = 2.0 ** 30, 2.0 ** 5    # (a product scale of 2^35 also fits the one-limb level)
    words = _ct_words(env, (5 if form == "slice" else B, size), l)
    ct = g.upload_ct_batch(words, cs)
    if form == "mod_switched":
        ct, words, l = g.mod_switch(ct), np.ascontiguousarray(words[:, :, :l - 1]), l - 1
    if form == "slice":
        ct, words = ct.slice(1, B), words[1:1 + B]
    rows = env.rng.uniform(-4, 4, (B, 8))
    pa, pm = g.encode_pt_array(rows, l, cs), g.encode_pt_array(rows.astype(np.float32), l, ps)
    wa, wm = pa.download_instances(), pm.download_instances()
    image = rows.astype(np.float32).astype(np.float64)
    for name, call, ocall, pt, pw, src in (("add_plain", g.add_plain, o.add_plain, pa, wa, rows), ("sub_plain", g.sub_plain, o.sub_plain, pa, wa, rows),
                                           ("multiply_plain", g.multiply_plain, o.multiply_plain, pm, wm, image)):
        out = call(ct, pt)
        assert out.batch == B and out.info() == (size, l, cs * ps if name == "multiply_plain" else cs)
        got = out.download()
        for b in range(B):
            one = call(ct.slice(b, 1), g.encode_pt(src[b], l, pt.scale)).download()
            assert np.array_equal(got[b], one), f"{name}: instance {b} differs from the single call"
            assert np.array_equal(got[b], ocall(np.ascontiguousarray(words[b]), pw[b])), f"{name}: instance {b} differs from the oracle"
    # a plaintext of batch 1 is still the operand every instance shares
    shared = g.encode_pt(rows[0], l, ps)
    got = g.multiply_plain(ct, shared).download()
    for b in range(B):
        assert np.array_equal(got[b], o.multiply_plain(np.ascontiguousarray(words[b]), shared.download()))
    one = g.encode_pt_array(rows[:1], l, ps)
    assert one.batch == 1 and np.array_equal(g.multiply_plain(ct, one).download(), got)


def test_a_batch_mismatch_is_refused(env1k):
    g, k = env1k.g, env1k.k
    l = k - 1
    ct3 = g.upload_ct_batch(_ct_words(env1k, (3, 2), l), SCALE)
    ct1 = g.upload_ct(_ct_words(env1k, (2,), l), SCALE)
    p2 = g.encode_pt_array(env1k.rng.uniform(-1, 1, (2, 8)), l, SCALE)
    p2m = g.encode_pt_array(env1k.rng.uniform(-1, 1, (2, 8)), l, 2.0 ** 5)
    msg = "plaintext batch differs from the ciphertext's"
    for ct in (ct3, ct1):
        assert _err(g.add_plain, ct, p2) == msg
        assert _err(g.sub_plain, ct, p2) == msg
        assert _err(g.multiply_plain, ct, p2m) == msg
        assert _err(g.weighted_sum, [ct, ct], [p2m, p2m]) == msg
        assert _err(g.elementwise_program, [ct, p2m], [(13, 0, 1)], [2]) == msg
        assert _err(g.elementwise_program, [ct, p2], [(11, 0, 1)], [2]) == msg


# ---- 3. weighted sums

@pytest.mark.parametrize("n", [3, 64])
def test_weighted_sum_mixes_shared_batched_and_unit_weights(env1k, n):
    env = env1k
    g, o, N, k = env.g, env.o, env.N, env.k
    l, B = k - 1, 3
    cs, ps = 2.0 ** 30, 2.0 ** 5
    kinds = ["batched", "shared", "one"] * (n // 3 + 1)
    kinds = kinds[:n]
    cts, pts, words, pwords, singles = [], [], [], [], []
    for kind in kinds:
        w = _ct_words(env, (B, 2), l)
        words.append(w)
        cts.append(g.upload_ct_batch(w, cs * ps if kind == "one" else cs))
        if kind == "batched":
            rows = env.rng.uniform(-4, 4, (B, 8))
            pts.append(g.encode_pt_array(rows, l, ps))
            pwords.append(pts[-1].download_instances())
            singles.append([g.encode_pt(rows[b], l, ps) for b in range(B)])
        elif kind == "shared":
            pts.append(g.encode_pt(env.rng.uniform(-4, 4, 8), l, ps))
            pwords.append(np.stack([pts[-1].download()] * B))
            singles.append([pts[-1]] * B)
        else:
            pts.append(None)
            pwords.append(None)
            singles.append([None] * B)
    out = g.weighted_sum(cts, pts)
    assert out.batch == B and out.info() == (2, l, cs * ps)
    got = out.download()
    for b in range(B):
        one = g.weighted_sum([c.slice(b, 1) for c in cts], [s[b] for s in singles]).download()
        assert np.array_equal(got[b], one), f"instance {b} differs from the single call"
        acc = None
        for j in range(n):
            wj = np.ascontiguousarray(words[j][b])
            term = wj if pwords[j] is None else o.multiply_plain(wj, pwords[j][b])
            acc = term if acc is None else o.add(acc, term)
        assert np.array_equal(got[b], acc), f"instance {b} differs from the oracle"


# ---- 4. the elementwise interpreter

def _ew_case(g, rng, primes, N, l, B):
    cs, ps = 2.0 ** 30, 2.0 ** 5
    draw = lambda prefix: np.stack([rng.integers(0, primes[i], size=tuple(prefix) + (N,), dtype=np.uint64) for i in range(l)], axis=len(prefix))
    x, y = g.upload_ct_batch(draw((B, 2)), cs), g.upload_ct_batch(draw((B, 2)), cs)
    wb = g.encode_pt_array(rng.uniform(-4, 4, (B, 8)).astype(np.float32), l, ps)
    ws = g.encode_pt(rng.uniform(-4, 4, 8), l, ps)
    ab = g.encode_pt_array(rng.integers(0, 9, size=(B, 8), dtype=np.uint8), l, cs * ps)
    # v5 = x * wb, v6 = y * ws, v7 = v5 + v6, v8 = v7 - ab, v9 = ab + v8 (plaintext first), v10 = -v9, v11 = x + y, v12 = v11 * wb
    ops = [(13, 0, 2), (13, 1, 3), (11, 5, 6), (12, 7, 4), (11, 4, 8), (10, 9, 9), (11, 0, 1), (13, 2, 11)]
    outs = g.elementwise_program([x, y, wb, ws, ab], ops, [10, 12, 8])
    v5, v6 = g.multiply_plain(x, wb), g.multiply_plain(y, ws)
    v8 = g.sub_plain(g.add(v5, v6), ab)
    want = [g.negate(g.add_plain(v8, ab)), g.multiply_plain(g.add(x, y), wb), v8]
    for got, ref in zip(outs, want):
        assert got.batch == B and got.info() == ref.info()
        assert np.array_equal(got.download(), ref.download())


def test_elementwise_program_one_coefficient_per_thread(env1k):
    _ew_case(env1k.g, env1k.rng, env1k.primes, env1k.N, env1k.k - 1, 3)


def test_elementwise_program_two_coefficients_per_thread():
    """8192 x 2 limbs x 64 instances = 2^20 coefficients: the launch shape with 16-byte accesses"""
    N = 8192
    primes = po.coeff_modulus_create(N, [60, 60, 60])
    g = backend.Context(N, primes)
    try:
        _ew_case(g, np.random.default_rng(12), primes, N, 2, 64)
    finally:
        g.close()


# ---- 5. the scheduler

def _sched_env(B):
    chain = "A"
    N, primes = ol.CHAINS[chain][0], ol.primes_of(chain)
    rng = np.random.default_rng(21)
    keys = ol.make_keys(chain, rng)
    g, o = backend.Context(N, primes), po.Oracle(N, primes)
    g.upload_relin_key(keys["relin"])
    for s, key in keys["galois"].items():
        g.upload_galois_key(g.galois_elt_from_step(s), key)
    return g, o, N, primes, rng, keys


def _run_and_walk(g, o, ops, placed, keys, B):
    """placed: {slot: ("ct", words [B][size][l][N], scale) | ("pt", words [l][N] or [B][l][N], scale, handle)}"""
    values = {}
    for s, v in placed.items():
        values[s] = g.upload_ct_batch(v[1], v[2]) if v[0] == "ct" else v[3]
    out = g.execute(ops, values)
    walks = []
    for b in range(B):
        inst = {s: (v[0], np.ascontiguousarray(v[1][b]) if v[0] == "ct" or v[1].ndim == 3 else v[1], v[2]) for s, v in placed.items()}
        walks.append(ol._walk_one(o, ops, inst, keys))
    return out, walks


def test_execute_takes_a_window_with_one_per_instance_weight():
    B = 3
    g, o, N, primes, rng, keys = _sched_env(B)
    try:
        l = len(primes) - 1
        cs, ps = 2.0 ** 30, 2.0 ** 5
        steps = [s for s in ol.steps_of("A") if s > 0][:2]
        x = ol.rand_words(rng, primes, N, (B, 2), l)
        w0 = g.encode_pt_array(rng.uniform(-4, 4, (B, 8)), l, ps)
        w1, w2 = (g.encode_pt(rng.uniform(-4, 4, 8), l, ps) for _ in range(2))
        placed = {0: ("ct", x, cs), 1: ("pt", w0.download_instances(), ps, w0), 2: ("pt", w1.download(), ps, w1), 3: ("pt", w2.download(), ps, w2)}
        F0, F1 = backend.OPF_FREE_SRC0, backend.OPF_FREE_SRC1
        ops = [(ol.ROTL, 4, 0, 0, steps[0], 0), (ol.ROTL, 5, 0, 0, steps[1], 0),
               (ol.MUL, 6, 0, 1, 0, 0), (ol.MUL, 7, 4, 2, 0, F0), (ol.MUL, 8, 3, 5, 0, F1),
               (ol.ADD, 9, 6, 7, 0, F0 | F1), (ol.ADD, 10, 9, 8, 0, F0 | F1)]
        out, walks = _run_and_walk(g, o, ops, placed, keys, B)
        got = out[10].download()
        assert out[10].batch == B
        for b in range(B):
            assert np.array_equal(got[b], walks[b][10][1]), f"instance {b}"
        # the same taps with shared weights only still take the fused window
        w3 = g.encode_pt(rng.uniform(-4, 4, 8), l, ps)
        placed[1] = ("pt", w3.download(), ps, w3)
        out, walks = _run_and_walk(g, o, ops, placed, keys, B)
        got = out[10].download()
        for b in range(B):
            assert np.array_equal(got[b], walks[b][10][1]), f"shared weights, instance {b}"
    finally:
        g.close()


def test_execute_defers_chains_with_per_instance_plaintexts():
    B = 3
    g, o, N, primes, rng, keys = _sched_env(B)
    try:
        l = len(primes) - 1
        cs, ps = 2.0 ** 30, 2.0 ** 5
        x, y = ol.rand_words(rng, primes, N, (B, 2), l), ol.rand_words(rng, primes, N, (B, 2), l)
        wb = g.encode_pt_array(rng.uniform(-4, 4, (B, 8)), l, ps)
        ab = g.encode_pt_array(rng.uniform(-4, 4, (B, 8)), l, cs * ps)
        ws = g.encode_pt(rng.uniform(-4, 4, 8), l, ps)
        placed = {0: ("ct", x, cs), 1: ("ct", y, cs), 2: ("pt", wb.download_instances(), ps, wb), 3: ("pt", ab.download_instances(), cs * ps, ab),
                  4: ("pt", ws.download(), ps, ws)}
        F0, F1 = backend.OPF_FREE_SRC0, backend.OPF_FREE_SRC1
        ops = [(ol.MUL, 5, 0, 2, 0, 0), (ol.MUL, 6, 4, 1, 0, 0), (ol.SUB, 7, 5, 6, 0, F0 | F1), (ol.ADD, 8, 3, 7, 0, F1),
               (ol.SUB, 9, 8, 3, 0, F0), (ol.NEG, 10, 9, 0, 0, F0), (ol.MUL, 11, 10, 2, 0, F0)]
        # scales: v5, v6 at cs ps; v8 adds ab at cs ps; v11 multiplies by wb once more (cs ps^2)
        out, walks = _run_and_walk(g, o, ops, placed, keys, B)
        got = out[11].download()
        assert out[11].batch == B and out[11].info() == (2, l, cs * ps * ps)
        for b in range(B):
            assert np.array_equal(got[b], walks[b][11][1]), f"instance {b}"
    finally:
        g.close()


# ---- 6. the product flow

VEC, N_FLOW, SCALE_BITS = 8, 1024, 30


def _program(N=N_FLOW):
    prog = EvaProgram('plainrows', vec_size=VEC)
    with prog:
        x, y, w = Input('x'), Input('y'), Input('w', False)
        Output('a', x * w + y)
        Output('b', (x << 1) * w + (x >> 1) * (w * w) + x * 0.5)
        Output('c', x - w)
        Output('d', w * 2 + 1)
    prog.set_input_scales(SCALE_BITS)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    params.poly_modulus_degree = N
    return compiled, params, sig


@pytest.fixture(scope="module")
def flow():
    compiled, params, sig = _program()
    pub, sec = generate_keys(params, 6)
    return compiled, sig, pub, sec


def _inputs(B, dtype=np.float64, seed=8):
    """The compiled program encodes w * w at scale 2^60 (beside x >> 1 at 2^30, to meet the other terms of `b` at 2^90).
    The device encoder's bound on a row v at scale s is mean |v| * s (its a-priori coefficient bound; device_encodable wants
    it at most 2^60): w in [-0.9, 0.9] or a 0 / 1 mask keeps mean |w * w| <= 1, so every row is encodable there."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(-2, 2, (B, VEC)), rng.uniform(-2, 2, (B, VEC))
    w = rng.integers(0, 2, size=(B, VEC), dtype=np.uint8) if dtype == np.uint8 else rng.uniform(-0.9, 0.9, (B, VEC)).astype(dtype)
    return x, y, w


def _as_lists(x, y, w):
    return [{'x': [float(v) for v in x[b]], 'y': [float(v) for v in y[b]], 'w': [float(v) for v in w[b]]} for b in range(len(x))]


@pytest.mark.parametrize("B,chunk", [(5, 2), (70, 64)])
def test_execute_batch_with_a_raw_input_that_differs_per_instance(flow, B, chunk):
    """On the parent commit the first execute_batch raises "unencrypted input w must be the same for every instance"."""
    compiled, sig, pub, sec = flow
    x, y, w = _inputs(B)
    rows = _as_lists(x, y, w)
    keep = pub.batch_chunk
    pub.batch_chunk = chunk
    try:
        encs = pub.encrypt_batch(rows, sig, device_sampling=True, seed=3)
        outs = pub.execute_batch(compiled, encs)
        assert len(outs) == B
        for b in range(B) if B == 5 else (0, 1, 63, 64, 69):
            _same(outs[b], oracle_execute(pub, compiled, encs[b]))
            _same(outs[b], pub.execute(compiled, encs[b]))
        got = sec.decrypt_batch(outs, sig)
        for b in range(B):
            mse = valuation_mse(got[b], evaluate(compiled, rows[b]))
            assert mse < 0.01, (b, mse)
            assert np.array_equal(np.array(got[b]['d']), w[b] * 2 + 1)
        # the same rows as arrays, w in each of the three types where it is integral, float32 / float64 otherwise
        for dtype in (np.float32, np.float64):
            wt = w.astype(dtype)
            lists = _as_lists(x, y, wt)
            want = pub.execute_batch(compiled, pub.encrypt_batch(lists, sig, device_sampling=True, seed=3))
            vb = pub.encrypt_array({'x': x, 'y': y}, sig, seed=3, plain_arrays={'w': wt})
            assert isinstance(vb, SEALValuationBatch) and sorted(vb.names()) == ['w', 'x', 'y']
            assert vb.plain_arrays()['w'].dtype == np.dtype(dtype) and np.array_equal(vb.plain_arrays()['w'], wt)
            assert vb[B - 1].get('w')[0] == "raw" and vb[B - 1].get('w')[4] == [float(v) for v in wt[B - 1]]
            s0 = pub.stack_stats()
            vouts = pub.execute_batch(compiled, vb)
            assert pub.stack_stats() == s0, "the array path stacks nothing"
            for b in range(B):
                _same(vouts[b], want[b])
            arr = sec.decrypt_array(vouts, sig)
            assert sorted(arr) == ['a', 'b', 'c', 'd'] and arr['d'].shape == (B, VEC) and arr['d'].dtype == np.float64
            assert np.array_equal(arr['d'], wt.astype(np.float64) * 2 + 1)
            lw = sec.decrypt_batch(want, sig)
            for n in ('a', 'b', 'c'):
                for b in range(B):
                    assert _bits_equal(arr[n][b], lw[b][n]), (n, b)
    finally:
        pub.batch_chunk = keep


def test_rows_cross_in_their_own_type(flow):
    """The same integral rows as uint8, float32 and float64: the program encodes the input w itself at n >= 1 nodes and
    values derived from it by raw arithmetic (w * w: float64 rows whatever w's type) at others, once per group, so between
    two types the bytes of a call differ by n rows of w at the difference of their item sizes and by nothing else."""
    compiled, sig, pub, sec = flow
    B = 5
    x, y, w = _inputs(B, np.uint8)
    sent, outs = {}, {}
    for dtype in (np.uint8, np.float32, np.float64):
        vb = pub.encrypt_array({'x': x, 'y': y}, sig, seed=3, plain_arrays={'w': w.astype(dtype)})
        assert vb.plain_arrays()['w'].dtype == np.dtype(dtype)
        pub.execute_batch(compiled, vb)   # the program's constants are on the device afterwards
        t0 = pub.transfer_stats()
        outs[dtype] = pub.execute_batch(compiled, vb)
        t1 = pub.transfer_stats()
        sent[dtype] = t1["h2d_bytes"] - t0["h2d_bytes"]
        assert t1["ct_uploads"] == t0["ct_uploads"] and t1["d2h_bytes"] == t0["d2h_bytes"]
    print({np.dtype(k).name: v for k, v in sent.items()})
    n, rest = divmod(sent[np.float64] - sent[np.float32], 4 * B * VEC)
    assert rest == 0 and n >= 1
    assert sent[np.float64] - sent[np.uint8] == 7 * n * B * VEC
    assert sent[np.uint8] >= n * B * VEC and (sent[np.uint8] - n * B * VEC) % (8 * B * VEC) == 0   # the rest: float64 rows
    want = pub.execute_batch(compiled, pub.encrypt_batch(_as_lists(x, y, w), sig, device_sampling=True, seed=3))
    for dtype in outs:
        for b in range(B):
            _same(outs[dtype][b], want[b])


def test_rows_that_are_all_equal_take_the_shared_path(flow):
    compiled, sig, pub, sec = flow
    B = 5
    x, y, w = _inputs(B)
    w[:] = w[0]
    rows = _as_lists(x, y, w)
    encs = pub.encrypt_batch(rows, sig, device_sampling=True, seed=3)
    outs = pub.execute_batch(compiled, encs)
    for b in range(B):
        _same(outs[b], pub.execute(compiled, encs[b]))
    vb = pub.encrypt_array({'x': x, 'y': y}, sig, seed=3, plain_arrays={'w': w})
    shared = pub.encrypt_array({'x': x, 'y': y, 'w': list(w[0])}, sig, seed=3)
    a, b_ = pub.execute_batch(compiled, vb), pub.execute_batch(compiled, shared)
    for b in range(B):
        _same(a[b], b_[b])
        _same(a[b], outs[b])


def test_dag_mode_equals_the_single_device_result(flow):
    compiled, sig, pub, sec = flow
    B = 5
    x, y, w = _inputs(B, seed=9)
    rows = _as_lists(x, y, w)
    ref = pub.execute_batch(compiled, pub.encrypt_batch(rows, sig, device_sampling=True, seed=2))
    pub2, sec2 = generate_keys(_program()[1], 6)   # same seed: same keys
    pub2.devices, pub2.shard_mode = [0, 0, 0], "dag"
    pub2.batch_chunk = 2
    outs = pub2.execute_batch(compiled, pub2.encrypt_batch(rows, sig, device_sampling=True, seed=2))
    for b in range(B):
        _same(outs[b], ref[b])


def test_seventy_instances_at_n_8192():
    compiled, params, sig = _program(8192)
    pub, sec = generate_keys(params, 6)
    B = 70
    x, y, w = _inputs(B, np.float32, seed=4)
    vb = pub.encrypt_array({'x': x, 'y': y}, sig, seed=3, plain_arrays={'w': w})
    outs = pub.execute_batch(compiled, vb)
    for b in (0, 63, 64, 69):
        _same(outs[b], oracle_execute(pub, compiled, vb[b]))
    arr = sec.decrypt_array(outs, sig)
    wd = w.astype(np.float64)
    assert np.abs(arr['a'] - (x * wd + y)).max() < 1e-2 and np.abs(arr['c'] - (x - wd)).max() < 1e-2
    assert np.array_equal(arr['d'], wd * 2 + 1)


# ---- 7. a row the device encoder cannot take

def test_a_row_the_device_encoder_cannot_take_names_the_input_and_the_instance(flow):
    compiled, sig, pub, sec = flow
    B = 5
    x, y, w = _inputs(B)
    w[3, 2] = np.inf
    encs = pub.encrypt_batch(_as_lists(x, y, w), sig, device_sampling=True, seed=3)
    keep = pub.batch_chunk
    pub.batch_chunk = 64
    try:
        with pytest.raises(RuntimeError, match="unencrypted input w, instance 3"):
            pub.execute_batch(compiled, encs)
        vb = pub.encrypt_array({'x': x, 'y': y}, sig, seed=3, plain_arrays={'w': w.astype(np.float32)})
        with pytest.raises(RuntimeError, match="unencrypted input w, instance 3"):
            pub.execute_batch(compiled, vb)
    finally:
        pub.batch_chunk = keep
