"""GPU: the collective relinearization key — evah_keygen_relin_round1 / _round2 at the C-ABI and the two
rounds through the public interface.

C-ABI.  Both rounds equal the host twins (relin_round1_host / relin_round2_host, which tests/test_relin_rounds_cpu.py
holds to the Python-integer model) word for word on [60] * 4 and [60, 30, 45, 50, 33, 60] at N in {1024 (exactly one block
of k_relin_round1, half a block of k_relin_round2 per row), 4096} for D in {1, k - 1}; on a chain of 10 primes at N = 1024,
whose 9 digits cross SEEDS_PER_LAUNCH (the seeds come from a device buffer); and on worst-case words — every aggregate
residue q_i - 1, every secret-key coefficient -1.  The transfer counters count what crossed.  Refusals carry their
messages and leave the context usable.

Public interface.  The device's shares equal a child process's with EVA_DEVICE_CLIENT=0.  A committee of 3 on [60] * 4 at
N = 4096 runs x * x + x and the README polynomial 3 x^2 + 5 x - 2 under the collective context and opens them by
decrypt_share / combine_shares at sigma = 40, and a batch of 3 through execute_batch; the ciphertext execute() returns
equals the oracle's walk of the same program with the same key words, bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from eva import EvaProgram, Input, Output, load
from eva.ckks import CKKSCompiler, CKKSParameters
from eva.seal import generate_keys
from eva_amd import _eva, backend
from oracle import pyoracle as po
from test_gpu_extremes import _same

pytestmark = pytest.mark.gpu

seal = _eva._seal
combine_public_contexts, combine_relin_shares, RelinShare = seal.combine_public_contexts, seal.combine_relin_shares, seal.RelinShare
round1_host, round2_host = seal._relin_round1_host, seal._relin_round2_host
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAINS = {"60x4": [60] * 4, "mixed": [60, 30, 45, 50, 33, 60], "ten": [50] * 9 + [60]}
SHAPES = [(N, chain) for N in (1 << 10, 1 << 12) for chain in ("60x4", "mixed")] + [(1 << 10, "ten")]


def _rand(rng, primes, N, prefix, nl):
    return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))


def _keys(rng, D):
    return np.frombuffer(rng.bytes(32 * D), dtype=np.uint8).reshape(D, 32).copy()


class _Case:
    """one context holding a random ternary secret key, with seeds, both key lists and a random aggregate for k - 1 digits"""

    def __init__(self, N, chain):
        self.N, self.primes = N, po.coeff_modulus_create(N, CHAINS[chain])
        self.k = len(self.primes)
        self.D = self.k - 1
        self.o = po.Oracle(N, self.primes)
        rng = self.rng = np.random.default_rng(N + 3 * self.k)
        self.s_ntt = self.secret(rng.integers(-1, 2, size=N))
        self.seeds, self.r1, self.r2 = _keys(rng, self.D), _keys(rng, self.D), _keys(rng, self.D)
        self.agg = _rand(rng, self.primes, N, (self.D, 2), self.k)
        self.g = backend.Context(N, self.primes)
        self.g.upload_secret_key(self.s_ntt)

    def secret(self, s):
        return np.stack([self.o.ntt(i, np.array([int(v) % q for v in s], dtype=np.uint64)) for i, q in enumerate(self.primes)])


@pytest.fixture(scope="module", params=SHAPES, ids=[f"N{N}_{c}" for N, c in SHAPES])
def case(request):
    p = _Case(*request.param)
    yield p
    p.g.close()


def test_both_rounds_equal_the_host_twins(case):
    p, g = case, case.g
    for D in sorted({1, p.D}):
        before = g.transfer_stats()
        got1 = g.keygen_relin_round1(p.seeds[:D], p.r1[:D])
        mid = g.transfer_stats()
        assert got1.shape == (D, 2, p.k, p.N)
        assert (mid[4] - before[4], mid[5] - before[5]) == (64 * D, got1.nbytes)
        _same(got1.reshape(2 * D, p.k, p.N), round1_host(p.N, p.primes, p.s_ntt, p.seeds[:D], p.r1[:D]).reshape(2 * D, p.k, p.N), f"round 1, D = {D}")
        agg = np.ascontiguousarray(p.agg[:D])
        got2 = g.keygen_relin_round2(agg, p.r1[:D], p.r2[:D])
        after = g.transfer_stats()
        assert got2.shape == (D, p.k, p.N)
        assert (after[4] - mid[4], after[5] - mid[5]) == (agg.nbytes + 64 * D, got2.nbytes)
        _same(got2, round2_host(p.N, p.primes, p.s_ntt, agg, p.r1[:D], p.r2[:D]), f"round 2, D = {D}")
    # a second call with the same keys gives the same words: nothing of the first stays behind in the scratch it reuses
    _same(g.keygen_relin_round1(p.seeds, p.r1).reshape(2 * p.D, p.k, p.N), got1.reshape(2 * p.D, p.k, p.N), "round 1 again")


def test_worst_case_words(case):
    p = case
    worst = np.empty((p.D, 2, p.k, p.N), dtype=np.uint64)
    for i, q in enumerate(p.primes):
        worst[:, :, i, :] = q - 1
    s_worst = p.secret(np.full(p.N, -1))
    h = backend.Context(p.N, p.primes)
    try:
        h.upload_secret_key(s_worst)
        _same(h.keygen_relin_round2(worst, p.r1, p.r2), round2_host(p.N, p.primes, s_worst, worst, p.r1, p.r2), "round 2 on q_i - 1 and s = -1")
        got1 = h.keygen_relin_round1(p.seeds, p.r1)
        _same(got1.reshape(2 * p.D, p.k, p.N), round1_host(p.N, p.primes, s_worst, p.seeds, p.r1).reshape(2 * p.D, p.k, p.N), "round 1 on s = -1")
    finally:
        h.close()
    # the random key's context on the worst aggregate
    _same(p.g.keygen_relin_round2(worst, p.r1, p.r2), round2_host(p.N, p.primes, p.s_ntt, worst, p.r1, p.r2), "round 2 on q_i - 1")


def _err(fn, *args):
    with pytest.raises(backend.EvaHipError) as e:
        fn(*args)
    return str(e.value)


def test_refusals_leave_the_context_usable():
    p = _Case(1 << 10, "mixed")
    try:
        _refusals(p, p.g)
    finally:
        p.g.close()


def _refusals(p, g):
    lib, u8p = backend._lib, C.POINTER(C.c_uint8)
    D = p.D
    seeds, r1, r2 = (a.ctypes.data_as(u8p) for a in (p.seeds, p.r1, p.r2))
    out1, out2 = np.empty((D, 2, p.k, p.N), dtype=np.uint64), np.empty((D, p.k, p.N), dtype=np.uint64)
    raw1 = lambda *a: backend._chk(lib.evah_keygen_relin_round1(g.h, *a))
    raw2 = lambda *a: backend._chk(lib.evah_keygen_relin_round2(g.h, *a))
    assert _err(raw1, D, None, r1, backend._p(out1)) == "seed pointer is null"
    assert _err(raw1, D, seeds, None, backend._p(out1)) == "randomness key pointer is null"
    assert _err(raw1, D, seeds, r1, None) == "output pointer is null"
    assert _err(raw2, D, None, r1, r2, backend._p(out2)) == "key pointer is null"
    assert _err(raw2, D, backend._p(p.agg), None, r2, backend._p(out2)) == "randomness key pointer is null"
    assert _err(raw2, D, backend._p(p.agg), r1, None, backend._p(out2)) == "randomness key pointer is null"
    assert _err(raw2, D, backend._p(p.agg), r1, r2, None) == "output pointer is null"
    for bad in (0, p.k):
        assert _err(raw1, bad, seeds, r1, backend._p(out1)) == "invalid key digit count"
        assert _err(raw2, bad, backend._p(p.agg), r1, r2, backend._p(out2)) == "invalid key digit count"
    a2 = g.upload_ct(_rand(p.rng, p.primes, p.N, (2,), p.k - 1), 2.0 ** 30)
    g.capture_begin()
    try:
        neg = g.negate(a2)   # (an empty capture is no graph)
        assert "cannot be captured into a graph" in _err(g.keygen_relin_round1, p.seeds, p.r1)
        assert "cannot be captured into a graph" in _err(g.keygen_relin_round2, p.agg, p.r1, p.r2)
    finally:
        g.graph_free(g.capture_end())
    del neg
    bare = backend.Context(p.N, p.primes)
    try:
        assert _err(bare.keygen_relin_round1, p.seeds, p.r1) == "secret key not present"
        assert _err(bare.keygen_relin_round2, p.agg, p.r1, p.r2) == "secret key not present"
        bare.set_shard(0, 2)
        assert "limb shard" in _err(bare.keygen_relin_round1, p.seeds, p.r1)
        assert "limb shard" in _err(bare.keygen_relin_round2, p.agg, p.r1, p.r2)
    finally:
        bare.close()
    # the context still works, and counts only what the calls that ran moved
    before = g.transfer_stats()
    _same(g.keygen_relin_round2(p.agg, p.r1, p.r2), round2_host(p.N, p.primes, p.s_ntt, p.agg, p.r1, p.r2), "after the refusals")
    after = g.transfer_stats()
    assert (after[4] - before[4], after[5] - before[5]) == (p.agg.nbytes + 64 * D, out2.nbytes)


# ---- through the public interface
COMMON = bytes(range(90, 122))
E2E_N, E2E_BITS, SIGMA = 1 << 12, [60] * 4, 40

_CHILD = """
import sys
sys.path.insert(0, 'tests')
from test_gpu_relin_rounds import twin_rounds
from eva import save
one, two = twin_rounds()
save(one, sys.argv[1])
save(two, sys.argv[2])
"""


def twin_rounds():
    """party 0's two shares of a committee of two on the mixed chain at N = 1024; the aggregate is formed on the host"""
    params = CKKSParameters(CHAINS["mixed"], set(), 1024)
    secs = [generate_keys(params, seed=11 + p, common_seed=COMMON)[1] for p in range(2)]
    before = secs[0].transfer_stats()
    eph, one = secs[0].relin_round1(seed=5)
    twin_rounds.d2h = secs[0].transfer_stats()["d2h_bytes"] - before["d2h_bytes"]
    agg = combine_relin_shares([one, secs[1].relin_round1(seed=6)[1]])
    return one, secs[0].relin_round2(eph, agg, seed=7)


def test_device_shares_equal_the_host_twin_child(tmp_path):
    paths = [str(tmp_path / "host.one"), str(tmp_path / "host.two")]
    child_env = dict(os.environ, PYTHONPATH=ROOT, EVA_DEVICE_CLIENT="0")
    out = subprocess.run([sys.executable, "-c", _CHILD] + paths, cwd=ROOT, env=child_env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    dev = twin_rounds()
    assert twin_rounds.d2h == dev[0].words().nbytes, "the device made the share"
    for path, d, rnd in zip(paths, dev, (1, 2)):
        host = load(path)
        assert isinstance(host, RelinShare) and (host.round, host.n_digits, host.N, list(host.primes)) == (rnd, d.n_digits, d.N, list(d.primes))
        _same(d.words().reshape(-1, 6, 1024), host.words().reshape(-1, 6, 1024), f"round {rnd}: device against the host twin")


def _compile(build, scale_bits, name):
    prog = EvaProgram(name, vec_size=64)
    with prog:
        Output("y", build(Input("x")))
    prog.set_input_scales(scale_bits)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    return compiled, params, sig


def _committee(params, P=3):
    """P parties with a common seed, both rounds, the collective context with its key"""
    pairs = [generate_keys(params, seed=70 + p, common_seed=COMMON) for p in range(P)]
    r1 = [sec.relin_round1() for _, sec in pairs]
    agg = combine_relin_shares([s for _, s in r1])
    r2 = [sec.relin_round2(r1[p][0], agg) for p, (_, sec) in enumerate(pairs)]
    col = combine_public_contexts([pub for pub, _ in pairs], relin_round1=agg, relin_round2=r2)
    assert col.collective and col.has_relin_key
    return pairs, col


@pytest.fixture(scope="module")
def committee():
    """three parties on [60] * 4 at N = 4096.  Both programs compile to chains of 60-bit primes only — x * x + x at input
    scale 2^50 to [60, 60, 60] without a rescale, the README polynomial at 2^30 to [60, 60, 60] with one rescale by a 60-bit
    prime — so the chain [60] * 4 serves both with one prime to spare"""
    square = _compile(lambda x: x * x + x, 50, "square_plus")
    poly = _compile(lambda x: 3 * x ** 2 + 5 * x - 2, 30, "readme")
    for _, params, _ in (square, poly):
        assert list(params.prime_bits) == [60, 60, 60]
    params = square[1]
    params.prime_bits = list(E2E_BITS)
    params.poly_modulus_degree = E2E_N
    pairs, col = _committee(params)
    return square, poly, pairs, col


def _flood_bound(P, scale):
    # N P 2^sigma / scale for the flood; 1e-6 covers the encryption's noise, the encoder's rounding and the FFT's FP64 error
    return E2E_N * P * 2.0 ** SIGMA / scale + 1e-6


def _open(col, pairs, out, sig, sigma=SIGMA):
    shares = [sec.decrypt_share(out, sigma) for _, sec in pairs]
    return col.combine_shares(out, shares, sig)["y"]


def _plain_under_the_sum(pairs, col, out):
    """the decryption of out["y"] under s = sum_p s_p, which only a test can form: the oracle's decrypt and decode"""
    primes = [int(q) for q in col.primes]
    o = po.Oracle(E2E_N, primes)
    s = np.stack([np.array(sum(sec._secret_key_ntt()[i].astype(object) for _, sec in pairs) % q, dtype=np.uint64) for i, q in enumerate(primes)])
    kind, size, limbs, scale, words = out.get("y")
    ct = np.asarray(words, dtype=np.uint64).reshape(size, limbs, E2E_N)
    return o.decode(o.decrypt(ct, s), scale)[:64]


def test_square_plus_x_under_the_collective_key(committee):
    (compiled, _, sig), _, pairs, col = committee
    xs = np.random.default_rng(0).uniform(-1, 1, 64)
    out = col.execute(compiled, col.encrypt({"x": xs.tolist()}, sig))
    kind, size, limbs, scale, _ = out.get("y")
    assert (size, limbs, scale) == (2, len(E2E_BITS) - 1, 2.0 ** 100)
    got = np.array(_open(col, pairs, out, sig))
    diff, bound = float(np.abs(got - (xs * xs + xs)).max()), _flood_bound(3, scale)
    print(f"x * x + x under the collective key, N = {E2E_N}, {E2E_BITS}, sigma = {SIGMA}: largest slot difference {diff:.3e}, bound {bound:.3e}")
    assert 0 < diff <= bound
    # two of three parties open nothing; one party alone decrypts noise
    shares = [sec.decrypt_share(out, SIGMA) for _, sec in pairs[:2]]
    assert float(np.abs(np.array(col.combine_shares(out, shares, sig)["y"]) - (xs * xs + xs)).max()) > 1.0
    assert float(np.abs(np.array(pairs[0][1].decrypt(out, sig)["y"]) - (xs * xs + xs)).max()) > 1.0


def test_readme_polynomial_under_the_collective_key(committee):
    _, (compiled, _, sig), pairs, col = committee
    xs = np.random.default_rng(1).uniform(-1, 1, 64)
    want = 3 * xs ** 2 + 5 * xs - 2
    out = col.execute(compiled, col.encrypt({"x": xs.tolist()}, sig))
    kind, size, limbs, scale, _ = out.get("y")
    assert size == 2 and scale == 2.0 ** 30
    got = np.array(_open(col, pairs, out, sig))
    diff, bound = float(np.abs(got - want).max()), _flood_bound(3, scale)
    print(f"3 x^2 + 5 x - 2 under the collective key, sigma = {SIGMA}, scale 2^30: largest slot difference {diff:.3e}, bound {bound:.3e}")
    assert 0 < diff <= bound
    # At scale 2^30 a flood of 40 bits leaves that bound above the values themselves, so what the relinearization did is
    # read off the plain decryption under the sum of the secrets as well, and off an opening whose flood fits the scale.
    # Tolerance ("what a relinearization costs"): the program relinearizes after its rescale, at scale 2^30
    # and l = 2, where the hard bound is far above the values, so the tolerance is five standard deviations of the slot the
    # cost concentrates in.  A digit d_J is a residue in [0, q_J): its mean q_J / 2 meets the key's noise E_J at the slot's
    # root zeta as (q_J / 2) |2 / (1 - zeta)| |E_J(zeta)| / P_special, and |2 / (1 - zeta)| reaches 2 N / pi at slot 0.
    # E_J(zeta) sums N coefficients of variance 2 N (2 P / 3) (10.5 P): s and u sums of P ternaries, e0 and e1 sums of P
    # errors of variance 10.5.  Every prime has 60 bits, so q_J / P_special is 1.  The inputs' own encryption noise and the
    # encoder's rounding add 0.01 at most (2.5e-5 per slot of x, the polynomial's derivative below 11).
    P, l = 3, limbs
    assert l == 2
    sd_E = np.sqrt(E2E_N * 2 * E2E_N * (2 * P / 3) * (10.5 * P))
    tol = l * (E2E_N / np.pi) * 5 * sd_E / scale + 0.01
    plain = _plain_under_the_sum(pairs, col, out)
    print(f"plain decryption under the sum of the secrets: largest slot difference {float(np.abs(plain - want).max()):.3e}, tolerance {tol:.3e}")
    assert tol < 0.6 and float(np.abs(plain - want).max()) <= tol
    # a flood that fits the scale: N P 2^8 / 2^30 from the plain decryption, hard
    low = np.array(_open(col, pairs, out, sig, sigma=8))
    flood8 = E2E_N * P * 2.0 ** 8 / scale
    assert float(np.abs(low - plain).max()) <= flood8 + 1e-9
    assert float(np.abs(low - want).max()) <= tol + flood8


def test_a_batch_of_3_through_execute_batch(committee):
    (compiled, _, sig), _, pairs, col = committee
    xs = np.random.default_rng(2).uniform(-1, 1, (3, 64))
    outs = col.execute_batch(compiled, col.encrypt_array({"x": xs}, sig, seed=2))
    assert sum(outs.segments("y")) == 3
    shares = [sec.decrypt_share(outs, SIGMA, seed=5 + p) for p, (_, sec) in enumerate(pairs)]
    got = col.combine_shares(outs, shares, sig)["y"]
    scale = outs[0].get("y")[3]
    assert got.shape == (3, 64)
    diff, bound = float(np.abs(got - (xs * xs + xs)).max()), _flood_bound(3, scale)
    print(f"batch of 3: largest slot difference {diff:.3e}, bound {bound:.3e}")
    assert 0 < diff <= bound


def test_execute_equals_the_oracle_walk_bit_for_bit():
    """the README polynomial on the chain the compiler chose: its walk goes through the fused Mul -> Rescale -> Relinearize form"""
    from eva_amd._eva import Op
    from oracle_executor import OracleExecutor
    compiled, params, sig = _compile(lambda x: 3 * x ** 2 + 5 * x - 2, 30, "readme")
    params.poly_modulus_degree = E2E_N
    pairs, col = _committee(params, P=2)
    enc = col.encrypt({"x": [i / 64.0 for i in range(64)]}, sig)
    out = col.execute(compiled, enc)
    ref = OracleExecutor(col).execute(compiled, enc)["y"]
    kind, size, limbs, scale, words = out.get("y")
    assert scale == ref.scale
    _same(np.asarray(words, dtype=np.uint64).reshape(ref.data.shape), ref.data, "execute() under the collective key against the oracle's walk")
    ops = [d["op"] for d in compiled._dump()]
    assert Op.Mul in ops and Op.Rescale in ops and Op.Relinearize in ops
