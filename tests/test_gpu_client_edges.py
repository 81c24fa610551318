"""GPU: the client kernels at every transform geometry and at their arithmetic edges (case builders and the derived
bound in tests/client_edges.py; tests/test_client_edges_cpu.py pins the oracle on the same cases).
A. k_fft_tile at every degree 2^10 .. 2^17 on dense inputs, both directions, against the oracle and the single calls
   (which reach 2^17 here for the first time).
B. crt_to_double on the sign decision, the word boundaries and the mixed per-word signs, at 1 to 61 limbs: constant
   polynomials against exact rationals and the oracle, and one polynomial of all the edges through the whole FFT.
C. k_enc_round / k_enc_round_many at the rounding threshold 2^52, at multiples of a prime of both signs and at -0.0,
   against Python integers; and the refusal of what the kernels cannot represent.
D. k_sample_small at exactly one tile, at four and at 64 tiles per polynomial, against the host twin.
Every comparison is bit for bit, except B1's bound, which client_edges.b1_bound derives."""
import numpy as np
import pytest

import client_edges as ce
from eva_amd import _eva
from oracle import pyoracle as po
from test_gpu_client_batch import SCALE, _Env, _bits_equal, _err

pytestmark = pytest.mark.gpu

sampled_small = _eva._seal._sampled_small
REFUSED = "encoded values are too large"


@pytest.fixture(scope="module")
def geo(request):
    """a context of its own per degree, with a short chain (the mixed 30 / 40 / 41-bit primes at 2^10)"""
    logn = request.param
    e = _Env(1 << logn, [40, 30, 40, 41] if logn == 10 else [60, 40, 60])
    yield e
    e.g.close()


every_degree = pytest.mark.parametrize("geo", range(10, 18), indirect=True, ids=lambda n: f"2^{n}")


def _zero_key(e):
    """with s = 0 and e = 0 the symmetric call's c0 is the plaintext itself"""
    e.g.upload_secret_key(np.zeros((e.k, e.N), dtype=np.uint64))


def _plaintexts_many(e, values, l, scale=SCALE):
    """the NTT-form plaintexts [batch][l][N] of the batched encoder, read as c0 under the all-zero key"""
    batch = len(values)
    seeds = [bytes([b + 1]) * 32 for b in range(batch)]
    ct = e.g.encode_encrypt_symmetric_many(values, l, scale, np.zeros((batch, e.N), dtype=np.int8), seeds)
    assert ct.batch == batch and ct.info() == (2, l, scale)
    return ct.download().reshape(batch, 2, l, e.N)[:, 0]


# ---- A. every transform geometry, dense inputs

@every_degree
def test_encoder_at_every_degree_on_dense_values(geo):
    e = geo
    _zero_key(e)
    values = ce.dense_values(e.rng, e.N // 2)
    for l in sorted({1, e.k - 1}):
        got = _plaintexts_many(e, values, l)
        for b in range(2):
            want = e.o.encode(l, values[b], SCALE)
            assert np.array_equal(got[b], want), f"batched encoder: instance {b}, l={l}"
            assert np.array_equal(e.g.encode_pt(values[b], l, SCALE).download(), want), f"single encoder: instance {b}, l={l}"


@every_degree
def test_decoder_at_every_degree_on_dense_inputs(geo):
    e = geo
    g, o, N = e.g, e.o, e.N
    g.upload_secret_key(e.sk)
    for l in sorted({1, e.k - 1}):
        # two ciphertexts of uniformly random residues and one of an encoded message of mixed magnitudes
        data = [np.stack([e.rand_poly(l), e.rand_poly(l)]) for _ in range(2)]
        data.append(ce.hide(o, l, e.sk, o.encode(l, ce.dense_values(e.rng, N // 2)[1], SCALE), e.rng))
        cts = [g.upload_ct(d, SCALE) for d in data]
        got = g.decrypt_decode_many(cts, N // 2)
        for b, d in enumerate(data):
            want = o.decode(o.decrypt(d, e.sk), SCALE)
            assert _bits_equal(got[b], want), f"batched decoder: ciphertext {b}, l={l}"
            assert _bits_equal(g.decrypt_decode(cts[b], N // 2), want), f"single decoder: ciphertext {b}, l={l}"


# ---- D. sampler geometry: N / 2048 tiles per polynomial

one_four_and_64_tiles = pytest.mark.parametrize("geo", [11, 13, 17], indirect=True, ids=lambda n: f"2^{n}")


def _twin(keys, N, polys):
    return np.array([[sampled_small(k, p, N) for p in polys] for k in keys], dtype=np.int8).reshape(len(keys), len(polys), N)


@one_four_and_64_tiles
def test_sampled_calls_equal_the_calls_on_the_twins_polynomials(geo):
    e = geo
    g, N = e.g, e.N
    g.upload_secret_key(e.sk)
    values = e.rng.uniform(-4, 4, (2, 8))
    rkeys = [e.rng.integers(0, 256, size=32, dtype=np.uint8).tobytes(), bytes(32)]
    seeds = [bytes([7]) * 32, bytes([9]) * 32]
    ct = g.encode_encrypt_sampled_many(values, 1, SCALE, rkeys)
    want = g.encode_encrypt_many(values, 1, SCALE, _twin(rkeys, N, (0, 1, 2)))
    assert ct.batch == 2 and ct.info() == (2, 1, SCALE)
    assert np.array_equal(ct.download(), want.download()), "public key"
    ct = g.encode_encrypt_symmetric_sampled_many(values, 1, SCALE, rkeys, seeds)
    want = g.encode_encrypt_symmetric_many(values, 1, SCALE, _twin(rkeys, N, (1,))[:, 0], seeds)
    assert np.array_equal(ct.download(), want.download()), "secret key"


# ---- B. the recomposition at its edges

@pytest.fixture(scope="module")
def chain(request):
    N, bits, scale_bits = request.param
    e = _Env(N, bits)
    e.scale = 2.0 ** scale_bits
    e.bits = bits
    yield e
    e.g.close()


RECOMP_CASES = ce.recomp_cases(po.coeff_modulus_create)


@pytest.mark.parametrize("chain,chunk", RECOMP_CASES, indirect=["chain"], ids=[ce.case_id(c) for c in RECOMP_CASES])
def test_constant_polynomials_at_the_recomposition_edges(chain, chunk):
    """B1.  64 ciphertexts per call; instance b encrypts the constant polynomial x_b, whose special FFT copies the
    recomposed double of coefficient 0 to every slot.  So every slot of an instance carries one double, that double is
    the oracle's bit for bit, and it lies within the derived bound client_edges.b1_bound = 2 (l + 1) 2^-53 S / scale of
    the exact rational centered(x_b) / scale (one rounding per word conversion and one per addition, S = sum of
    |accumulated word| 2^(64 w); the derivation is in b1_bound's docstring, nothing is measured).  At x = h and
    x = h + 1 the values are about +-Q / (2 scale), orders above the bound: the sign decision is what is tested."""
    e = chain
    g, o, N, l = e.g, e.o, e.N, e.k - 1
    every = ce.edge_values(e.primes[:l], np.random.default_rng(l))
    xs = every[64 * chunk:64 * chunk + 64]
    rng = np.random.default_rng(100 * l + chunk)
    data = ce.constant_cts(o, l, e.sk, xs, rng)
    got = g.decrypt_decode_many([g.upload_ct(d, e.scale) for d in data], N // 2)
    ce.check_constant_decodes(xs, got, e.primes[:l], e.scale, "device")
    for b, d in enumerate(data):
        assert _bits_equal(got[b], o.decode(o.decrypt(d, e.sk), e.scale)), f"oracle: x = {xs[b]:#x}"


@pytest.mark.parametrize("chain", ce.RECOMP_CHAINS, indirect=True, ids=ce.chain_id)
def test_one_polynomial_of_all_the_edges(chain):
    """B2.  the N coefficients cycle through the edge list; single and batched call, at the working scale and just
    inside "scale out of bounds" where that scale is a finite double"""
    e = chain
    g, o, N, l = e.g, e.o, e.N, e.k - 1
    every = ce.edge_values(e.primes[:l], np.random.default_rng(l))
    poly = ce.poly_ct(o, l, e.sk, ce.cycled(every, N), e.rng)
    other = np.stack([e.rand_poly(l), e.rand_poly(l)])
    top = sum(e.bits[:l]) - 8
    for scale in [e.scale] + ([2.0 ** top] if top < 1024 else []):
        want = o.decode(o.decrypt(poly, e.sk), scale)
        ct, ct2 = g.upload_ct(poly, scale), g.upload_ct(other, scale)
        assert _bits_equal(g.decrypt_decode(ct, N // 2), want), f"single call at scale {scale:g}"
        got = g.decrypt_decode_many([ct2, ct], N // 2)
        assert _bits_equal(got[1], want), f"batched call at scale {scale:g}"
        assert _bits_equal(got[0], o.decode(o.decrypt(other, e.sk), scale))


# ---- C. the encoder's rounding at its edges

@pytest.fixture(scope="module")
def enc(request):
    e = _Env(*request.param)
    _zero_key(e)
    yield e
    e.g.close()


encoder_chains = pytest.mark.parametrize("enc", ce.ENCODER_CHAINS, indirect=True, ids=lambda c: f"N{c[0]}")


def _encoder_cases(e):
    """(m, value): the list of client_edges.encoder_cases and -0.0.  A constant m / scale has the coefficient bound |m|
    exactly, so the whole list, up to 2^62 - 2^9, is inside the refusal's rule."""
    scale = 2.0 ** ce.ENC_SCALE_BITS
    cases = [(m, m / scale) for m in ce.encoder_cases(e.primes)] + [(0, -0.0)]
    assert all(ce.device_accepts([v], e.N, scale) for _, v in cases)
    return cases, scale


@encoder_chains
def test_single_encoder_rounds_the_edge_constants(enc):
    e = enc
    g, N, l = e.g, e.N, e.k - 1
    cases, scale = _encoder_cases(e)
    for m, v in cases:
        want = ce.constant_plaintext(m, e.primes, l, N)
        assert np.array_equal(g.encode_pt([v], l, scale).download(), want), f"m = {m} (value {v!r})"
        assert np.array_equal(e.o.encode(l, np.full(N // 2, v), scale), want), f"oracle: m = {m}"


@encoder_chains
def test_batched_encoder_rounds_the_edge_constants(enc):
    e = enc
    N, l = e.N, e.k - 1
    cases, scale = _encoder_cases(e)
    _zero_key(e)
    while len(cases) % 64:   # batches of 64: the last one is filled up with random multiples of 2^9 below 2^62
        m = int(e.rng.integers(-(1 << 53) + 1, 1 << 53)) << 9
        cases.append((m, m / scale))
    for at in range(0, len(cases), 64):
        batch = cases[at:at + 64]
        got = _plaintexts_many(e, np.array([[v] for _, v in batch]), l, scale)
        for b, (m, v) in enumerate(batch):
            want = ce.constant_plaintext(m, e.primes, l, N)
            assert np.array_equal(got[b], want), f"instance {at + b}: m = {m} (value {v!r})"
            assert np.array_equal(e.o.encode(l, np.full(N // 2, v), scale), want), f"oracle: m = {m}"


def test_the_five_encoding_calls_refuse_what_the_kernel_cannot_represent():
    N, bits = ce.ENCODER_CHAINS[0]
    e = _Env(N, bits)
    try:
        g, l, B = e.g, e.k - 1, 3
        _zero_key(e)
        keys = [bytes([b + 1]) * 32 for b in range(B)]
        no_error = np.zeros((B, N), dtype=np.int8)
        calls = {
            "evah_pt_encode": lambda v: g.encode_pt(v[-1], l, SCALE),
            "evah_encode_encrypt_many": lambda v: g.encode_encrypt_many(v, l, SCALE, e.small(B)),
            "evah_encode_encrypt_symmetric_many": lambda v: g.encode_encrypt_symmetric_many(v, l, SCALE, no_error, keys),
            "evah_encode_encrypt_sampled_many": lambda v: g.encode_encrypt_sampled_many(v, l, SCALE, keys),
            "evah_encode_encrypt_symmetric_sampled_many": lambda v: g.encode_encrypt_symmetric_sampled_many(v, l, SCALE, keys, keys),
        }
        dense = e.rng.uniform(-1, 1, N // 2)
        dense *= 2.0 ** 62 / ce.coeff_bound(dense, N, SCALE)   # the coefficient bound of `dense` is now 2^62 up to rounding

        def batch_of(last):
            v = np.tile(e.rng.uniform(-1, 1, len(last)), (B, 1))
            v[-1] = last
            return v

        top = (1 << 62) - (1 << 9)   # the largest double below 2^62
        below = [np.array([top / SCALE]), dense * (1 - 2.0 ** -20)]
        above = [np.array([2.0 ** 32]), dense * (1 + 2.0 ** -20), np.array([2.0 ** 34]), np.array([1e300])]
        bad = []
        for x in (np.nan, np.inf, -np.inf):
            v = e.rng.uniform(-1, 1, 8)
            v[5] = x
            bad.append(v)
        assert ce.coeff_bound(below[0], N, SCALE) == top and ce.coeff_bound(above[0], N, SCALE) == 2.0 ** 62
        assert all(ce.device_accepts(v, N, SCALE) for v in below) and not any(ce.device_accepts(v, N, SCALE) for v in above + bad)
        one = ce.constant_plaintext(1 << 30, e.primes, l, N)
        for name, call in calls.items():
            for v in above + bad:
                assert _err(call, batch_of(v)) == REFUSED, (name, v[:8])
                assert np.array_equal(g.encode_pt([1.0], l, SCALE).download(), one), f"{name}: the call after a refusal"
            for v in below:
                out = call(batch_of(v))
                assert out.info() == ((l, SCALE) if name == "evah_pt_encode" else (2, l, SCALE)), name
        # what was accepted just below the bound is encoded right
        assert np.array_equal(g.encode_pt(below[0], l, SCALE).download(), ce.constant_plaintext(top, e.primes, l, N))
        want = e.o.encode(l, below[1], SCALE)
        assert np.array_equal(g.encode_pt(below[1], l, SCALE).download(), want)
        assert np.array_equal(_plaintexts_many(e, batch_of(below[1]), l)[-1], want)
    finally:
        e.g.close()
