"""CPU: the client paths at their arithmetic edges (tests/client_edges.py), the part that needs no GPU.
The oracle's recomposition (punctured products) against exact rationals on the sign decision, the word boundaries and
the mixed per-word signs, which pins the reference test_gpu_client_edges.py compares the device with; the host decoder
(Garner digits, EVA_DEVICE_CLIENT=0) on the same ciphertexts against the oracle as float64 bit patterns; and the
encoder's rounding cases through the oracle and the host encoder against Python integers."""
import numpy as np
import pytest

import client_edges as ce
from eva.seal import generate_keys
from eva_amd import _eva
from oracle import pyoracle as po
from test_decode_parity import _bits_equal, _flow


@pytest.fixture(autouse=True)
def _host_client(monkeypatch):
    monkeypatch.setenv("EVA_DEVICE_CLIENT", "0")


def _keys(N, bits):
    """a key pair on the chain `bits` with a signature of N / 2 slots, and the oracle of the same primes"""
    _, params, sig = _flow(N // 2, N, 30)
    params.prime_bits = list(bits)
    pub, sec = generate_keys(params, 31)
    primes = [int(q) for q in pub.primes]
    assert [q.bit_length() for q in primes] == list(bits)
    return pub, sec, sig, primes, po.Oracle(N, primes)


@pytest.mark.parametrize("case", ce.recomp_cases(po.coeff_modulus_create), ids=ce.case_id)
def test_oracle_and_host_recomposition_at_the_edges(case):
    (N, bits, scale_bits), chunk = case
    pub, sec, sig, primes, o = _keys(N, bits)
    assert primes == po.coeff_modulus_create(N, bits)
    l, scale = len(bits) - 1, 2.0 ** scale_bits
    sk = sec._secret_key_ntt()
    every = ce.edge_values(primes[:l], np.random.default_rng(l))
    xs = every[64 * chunk:64 * chunk + 64]
    rng = np.random.default_rng(100 * l + chunk)
    Q = ce.product(primes[:l])
    # B1: constant polynomials — the oracle against rationals, the host decoder against the oracle
    cts = ce.constant_cts(o, l, sk, xs, rng)
    wants = [o.decode(o.decrypt(ct, sk), scale) for ct in cts]
    ce.check_constant_decodes(xs, wants, primes[:l], scale, "oracle")
    val = _eva._seal.SEALValuation()
    for b, ct in enumerate(cts):
        val._set_cipher(f"c{b}", ct, scale)
    scales = []
    if chunk == 0:
        assert every[:7] == [0, 1, Q - 1, Q // 2 - 1, Q // 2, Q // 2 + 1, Q // 2 + 2]
        at = [w[0] for w in wants[:7]]
        assert at[0] == 0.0 and at[1] == 1.0 / scale and at[2] == -1.0 / scale and at[4] > 0 > at[5]
        # B2: one polynomial whose coefficients cycle through all the edges, through the whole FFT
        poly = ce.poly_ct(o, l, sk, ce.cycled(every, N), rng)
        scales = [scale] + ([2.0 ** (sum(bits[:l]) - 8)] if sum(bits[:l]) - 8 < 1024 else [])
        for j, s in enumerate(scales):
            val._set_cipher(f"p{j}", poly, s)
    got = sec.decrypt(val, sig)
    for b, want in enumerate(wants):
        assert _bits_equal(got[f"c{b}"], want), f"host decoder: constant x = {xs[b]:#x}"
    for j, s in enumerate(scales):
        assert _bits_equal(got[f"p{j}"], o.decode(o.decrypt(poly, sk), s)), f"host decoder: edge polynomial at scale {s:g}"


@pytest.mark.parametrize("cfg", ce.ENCODER_CHAINS, ids=lambda c: f"N{c[0]}")
def test_oracle_and_host_encoder_round_the_edge_constants(cfg):
    N, bits = cfg
    _, params, _ = _flow(8, N, 30)
    params.prime_bits = list(bits)
    pub, _ = generate_keys(params, 2)
    primes = [int(q) for q in pub.primes]
    o = po.Oracle(N, primes)
    l, scale = len(bits) - 1, 2.0 ** ce.ENC_SCALE_BITS
    ms = ce.encoder_cases(primes)
    assert {0, 1, -1, 1 << 52, -(1 << 52), (1 << 62) - (1 << 9), primes[1], -primes[1]} <= set(ms)
    cases = [(m, m / scale) for m in ms] + [(0, -0.0)]
    for m, v in cases:
        assert v * scale == m
        want = ce.constant_plaintext(m, primes, l, N)
        assert np.array_equal(o.encode(l, np.full(N // 2, v), scale), want), f"oracle: m = {m}"
        assert np.array_equal(pub._encode([v], ce.ENC_SCALE_BITS, 0), want), f"host encoder: m = {m}"


def test_the_refusal_rule_restated():
    """the cases test_gpu_client_edges.py sends to the refusal straddle the rule by construction"""
    N, scale = 4096, 2.0 ** 30
    assert ce.coeff_bound([1.0], N, scale) == scale and ce.coeff_bound([0.5] * 8, N, scale) == scale / 2
    assert ce.device_accepts([2.0 ** 32 * (1 - 2.0 ** -53)], N, scale) and not ce.device_accepts([2.0 ** 32], N, scale)
    for bad in (float("nan"), float("inf"), float("-inf")):
        assert not ce.device_accepts([1.0, bad], N, scale)
    assert not ce.device_accepts([1e300], N, 1e300)
    # a constant m / scale has the bound |m| exactly: the whole list of encoder cases is inside the rule
    for m in ce.encoder_cases([1073479681]):
        assert ce.coeff_bound([m / scale], N, scale) == abs(m) and ce.device_accepts([m / scale], N, scale), m
