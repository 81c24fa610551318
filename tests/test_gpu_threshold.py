"""GPU: threshold decryption at the C-ABI — evah_decrypt_share_handles and evah_decrypt_combine_rows —
and through the public interface.

Shares.  For N in {1024 (half a FLOOD_TILE: the partial-tile branch of k_sample_flood), 4096 (two tiles)} and the chains
[60, 30, 45, 50, 33, 60] and [60] * 4: the device's share equals the host twin (decrypt_share_host, itself pinned to the
Python-integer model by tests/test_threshold_cpu.py) word for word at l in {1, 2, k - 1} through mod-switched views, for
n in {1, 3, 64} instances, through slices and unstacked views, for handles of a second context read in place, at
sigma in {1, 40, 62} on the mixed chain (|E| far above the 30-bit prime), and with every c1 residue and every secret-key
word q_i - 1.

Combination.  evah_decrypt_combine_rows equals m = c0 + sum_p h_p (numpy, exact) decoded by the oracle, bit for bit, for
P in {1, 2, 3, 9, 64} parties, float64 / float32 / uint8, host and device rows, a pitched destination, shares whose
residues are all q_i - 1 — on a context with no secret key.

The refusals leave the context usable.  The references of a context are computed once and shared by its tests."""
import os
import subprocess
import sys

import numpy as np
import pytest

import rekey_model as rkm
from eva import EvaProgram, Input, Output, load
from eva.ckks import CKKSCompiler
from eva.seal import combine_public_contexts, generate_keys
from eva_amd import _eva, backend
from eva_amd._eva._seal import DecryptionShares
from oracle import pyoracle as po
from test_gpu_device_arrays import _dest, _gaps_untouched, _u8_rule
from test_gpu_extremes import _same

pytestmark = pytest.mark.gpu

CHAINS = {"mixed": [60, 30, 45, 50, 33, 60], "60x4": [60] * 4}
CONTEXTS = [("N1024_mixed", 1 << 10, "mixed"), ("N1024_60x4", 1 << 10, "60x4"), ("small", 1 << 12, "60x4"), ("N4096_mixed", 1 << 12, "mixed")]
N_INST = 64
SCALE = 2.0 ** 30
share_host = _eva._seal._decrypt_share_host


def fkey(i):
    return bytes((i * 31 + j * 17 + 9) % 256 for j in range(32))


def _rand(rng, primes, N, prefix, nl):
    return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))


class _Case:
    """one context with a (uniform) secret-key share uploaded, 64 random size-2 ciphertexts at the top level, and the host
    twin's share of each (level, instance, sigma, key) computed once"""

    def __init__(self, name, N, chain):
        self.name, self.N, self.chain = name, N, chain
        self.primes = po.coeff_modulus_create(N, CHAINS[chain])
        self.k = len(self.primes)
        self.top = self.k - 1
        self.levels = sorted({1, 2, self.top})
        self.o = po.Oracle(N, self.primes)
        self.rng = np.random.default_rng(N + self.k)
        self.s = _rand(self.rng, self.primes, N, (), self.k)
        self.g = backend.Context(N, self.primes)
        self.g.upload_secret_key(self.s)
        self.cts = _rand(self.rng, self.primes, N, (N_INST, 2), self.top)
        self._ref = {}

    def want(self, l, b, sigma, key):
        if (l, b, sigma, key) not in self._ref:
            self._ref[l, b, sigma, key] = share_host(self.N, self.primes, self.s, np.ascontiguousarray(self.cts[b][:, :l]), sigma, key)
        return self._ref[l, b, sigma, key]

    def at_level(self, h, l):
        for _ in range(self.top - l):
            h = self.g.mod_switch(h)
        return h

    def sigma_max(self, l):
        Q = 1
        for q in self.primes[:l]:
            Q *= q
        return min(62, Q.bit_length() - 3)


@pytest.fixture(scope="module", params=CONTEXTS, ids=[c[0] for c in CONTEXTS])
def case(request):
    p = _Case(*request.param)
    yield p
    p.g.close()


def _err(fn, *a, **kw):
    with pytest.raises(backend.EvaHipError) as e:
        fn(*a, **kw)
    return str(e.value)


def test_shares_of_single_handles_at_every_level(case):
    p, g = case, case.g
    ups = [g.upload_ct(p.cts[b], SCALE) for b in range(N_INST)]
    for l in p.levels:
        hs = [p.at_level(h, l) for h in ups]   # l < top: mod-switched views, polynomial stride of the top level
        sigma = min(40, p.sigma_max(l))
        for n in (1, 3, 64):
            out = g.decrypt_share_handles(hs[:n], sigma, [fkey(b) for b in range(n)])
            assert (out.size, out.limbs, out.scale, out.batch) == (1, l, SCALE, n)
            got = out.download().reshape(n, l, p.N)
            for b in range(n):
                _same(got[b], p.want(l, b, sigma, fkey(b)), f"{p.name} l={l} n={n} instance {b}")
                assert all(int(got[b][i].max()) < p.primes[i] for i in range(l)), "canonical residues"


def test_slices_views_and_a_second_context(case):
    p, g = case, case.g
    l, sigma = p.top, 40
    B = g.upload_ct_batch(p.cts, SCALE)
    single = g.upload_ct(p.cts[2], SCALE)
    handles = [B.slice(59, 5), B.unstack(63), single]   # 5 + 1 + 1 instances in one call
    order = [59, 60, 61, 62, 63, 63, 2]
    out = g.decrypt_share_handles(handles, sigma, [fkey(100 + j) for j in range(7)])
    got = out.download().reshape(7, l, p.N)
    for j, b in enumerate(order):
        _same(got[j], p.want(l, b, sigma, fkey(100 + j)), f"{p.name} handle forms, row {j}")
    lower = g.mod_switch(B)   # the whole batch one level down, read through the stride of the top level
    if l > 1:
        out = g.decrypt_share_handles([lower.slice(10, 3)], 40, [fkey(j) for j in range(3)])
        got = out.download().reshape(3, l - 1, p.N)
        for j in range(3):
            _same(got[j], p.want(l - 1, 10 + j, 40, fkey(j)), f"{p.name} mod-switched slice, row {j}")
    other = backend.Context(p.N, p.primes)   # the device state of another key pair on the same GPU
    try:
        hs = [other.upload_ct(p.cts[b], SCALE) for b in range(3)]
        up0 = g.transfer_stats()
        out = g.decrypt_share_handles(hs, sigma, [fkey(b) for b in range(3)])
        up1 = g.transfer_stats()
        assert up1[0] == up0[0] and up1[4] - up0[4] == 3 * 32 and up1[5] == up0[5], "read in place: the keys go up, nothing else moves"
        got = out.download().reshape(3, l, p.N)
        for b in range(3):
            _same(got[b], p.want(l, b, sigma, fkey(b)), f"{p.name} second context, instance {b}")
    finally:
        other.close()


def test_noise_widths_and_worst_case_words(case):
    p, g = case, case.g
    if p.chain == "mixed":   # |E| up to 2^62 against the 30-bit prime: the Barrett step of the noise's residues
        up = g.upload_ct(p.cts[0], SCALE)
        for l in (2, p.top):
            h = p.at_level(up, l)
            for sigma in (1, 40, 62):
                got = g.decrypt_share_handles([h], sigma, [fkey(sigma)]).download().reshape(l, p.N)
                _same(got, p.want(l, 0, sigma, fkey(sigma)), f"{p.name} l={l} sigma={sigma}")
    # every c1 residue and every key word q_i - 1
    l = p.top
    worst = np.stack([np.stack([np.full(p.N, p.primes[i] - 1, dtype=np.uint64) for i in range(l)])] * 2)
    s_worst = np.stack([np.full(p.N, q - 1, dtype=np.uint64) for q in p.primes])
    h = backend.Context(p.N, p.primes)
    try:
        h.upload_secret_key(s_worst)
        for sigma in (1, 62):
            got = h.decrypt_share_handles([h.upload_ct(worst, SCALE)], sigma, [fkey(7)]).download().reshape(l, p.N)
            _same(got, share_host(p.N, p.primes, s_worst, worst, sigma, fkey(7)), f"{p.name} worst-case words, sigma={sigma}")
    finally:
        h.close()


def _model_rows(p, cts, shares, l, n_out, scale):
    """the oracle's decode of m = c0 + sum_p h_p per instance: float64 [n][n_out]"""
    rows = []
    for b in range(cts.shape[0]):
        m = np.empty((l, p.N), dtype=np.uint64)
        for i in range(l):
            q = np.uint64(p.primes[i])
            acc = cts[b][0][i].copy()
            for sh in shares:
                acc = (acc + sh[b][i]) % q   # both below q < 2^61: no wrap
            m[i] = acc
        rows.append(p.o.decode(m, scale)[:n_out])
    return np.stack(rows)


@pytest.mark.parametrize("P", [1, 2, 3, 9, 64])
def test_combine_equals_the_oracles_decode_of_the_sum(case, P):
    p = case
    pub = backend.Context(p.N, p.primes)   # no secret key: the public server's context
    try:
        rng = np.random.default_rng(P)
        l = p.top if P <= 3 else 2
        n = 3 if P <= 3 else 2
        cts = np.ascontiguousarray(p.cts[:n][:, :, :l])
        Q = 1
        for q in p.primes[:l]:
            Q *= q
        scale = 2.0 ** (Q.bit_length() - 10)   # random words decode to values of up to 2^9: every row type has something to show
        shares = [_rand(rng, p.primes, p.N, (n,), l) for _ in range(P)]
        if P == 2:   # every residue of a share q_i - 1
            shares[1] = np.stack([np.stack([np.full(p.N, p.primes[i] - 1, dtype=np.uint64) for i in range(l)])] * n)
        ct_h = pub.upload_ct_batch(cts, scale)
        sh_h = [pub.upload_ct_batch(sh.reshape(n, 1, l, p.N), scale) for sh in shares]
        n_out = p.N // 2 if P == 1 else 8
        want = _model_rows(p, cts, shares, l, n_out, scale)
        got = pub.decrypt_combine_rows([ct_h], sh_h, n_out, np.zeros((n, n_out)))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), f"{p.name} P={P}: float64 host rows"
        if P in (1, 3, 64):
            f32 = pub.decrypt_combine_rows([ct_h], sh_h, n_out, np.zeros((n, n_out), dtype=np.float32))
            assert np.array_equal(f32.view(np.uint32), want.astype(np.float32).view(np.uint32))
            u8 = pub.decrypt_combine_rows([ct_h], sh_h, n_out, np.zeros((n, n_out), dtype=np.uint8))
            assert np.array_equal(u8, _u8_rule(want))
            for dtype, ref in ((np.float64, want), (np.uint8, _u8_rule(want))):
                item = np.dtype(dtype).itemsize
                view, img = _dest(pub, n, n_out, dtype, (n_out + 3) * item)   # device rows with a pitch
                pub.decrypt_combine_rows([ct_h], sh_h, n_out, view)
                assert np.array_equal(view.to_numpy().view(f"u{item}"), ref.view(f"u{item}")) and _gaps_untouched(view, img)
            wide = np.full((n, n_out + 3), 7.0)   # host rows with a pitch
            pub.decrypt_combine_rows([ct_h], sh_h, n_out, wide[:, :n_out])
            assert np.array_equal(wide[:, :n_out].view(np.uint64), want.view(np.uint64)) and (wide[:, n_out:] == 7.0).all()
        if P == 3:   # single handles and a view beside the batched form: the same rows
            singles = [pub.upload_ct(cts[b], scale) for b in range(n)]
            again = pub.decrypt_combine_rows(singles, sh_h, n_out, np.zeros((n, n_out)))
            assert np.array_equal(again.view(np.uint64), want.view(np.uint64))
    finally:
        pub.close()


def test_share_then_combine_opens_the_message(case):
    """three key shares, a ciphertext under their sum: the combined shares decode to the message within N P 2^sigma / scale"""
    p, g = case, case.g
    P, l, sigma, scale = 3, p.top, 40, 2.0 ** 50
    rng = np.random.default_rng(11)
    ss = [_rand(rng, p.primes, p.N, (), p.k) for _ in range(P)]
    values = rng.uniform(-1, 1, p.N // 2)
    pt = p.o.encode(l, values, scale)
    c1 = _rand(rng, p.primes, p.N, (), l)
    c0 = np.empty_like(c1)
    for i in range(l):
        q = p.primes[i]
        s_sum = sum(s[i].astype(object) for s in ss) % q
        c0[i] = np.array((pt[i].astype(object) - c1[i].astype(object) * s_sum) % q, dtype=np.uint64)
    ct = np.stack([c0, c1])
    pub = backend.Context(p.N, p.primes)
    parties = [backend.Context(p.N, p.primes) for _ in range(P)]
    try:
        ct_h = pub.upload_ct(ct, scale)
        shares = []
        for j, party in enumerate(parties):
            party.upload_secret_key(ss[j])
            sh = party.decrypt_share_handles([ct_h], sigma, [fkey(50 + j)])   # the server's handle, read in place
            _same(sh.download().reshape(l, p.N), share_host(p.N, p.primes, ss[j], ct, sigma, fkey(50 + j)), f"party {j}")
            shares.append(sh)
        got = pub.decrypt_combine_rows([ct_h], shares, p.N // 2, np.zeros((1, p.N // 2)))[0]
        # N P 2^sigma / scale for the flood; 1e-6 covers the encoder's rounding (N / 2 / scale) and the FFT's FP64 error
        diff, bound = float(np.abs(got - values).max()), p.N * P * 2.0 ** sigma / scale + 1e-6
        print(f"{p.name}: largest slot difference at sigma = {sigma}: {diff:.3e}, bound {bound:.3e}")
        assert 0 < diff <= bound
    finally:
        for c in parties + [pub]:
            c.close()


def test_refusals_leave_the_context_usable(case):
    p, g = case, case.g
    l = p.top
    ct = g.upload_ct(p.cts[0], SCALE)
    k1 = [fkey(1)]
    size3 = g.upload_ct(np.concatenate([p.cts[0], p.cts[1][:1]]), SCALE)
    assert _err(g.decrypt_share_handles, [size3], 40, k1) == "decryption share expects a size-2 ciphertext (relinearize first)"
    size3.free()
    assert _err(g.decrypt_share_handles, [ct], 0, k1) == "smudge_bits must be 1..62"
    assert _err(g.decrypt_share_handles, [ct], 63, k1) == "smudge_bits must be 1..62"
    assert _err(g.decrypt_share_handles, [ct], 40, None) == "flooding keys are required"
    low = p.at_level(ct, 1)
    top = p.primes[0].bit_length() - 3
    g.decrypt_share_handles([low], top, k1)
    assert _err(g.decrypt_share_handles, [low], top + 1, k1) == "smudge_bits leaves no room at this level"
    other = g.upload_ct(np.ascontiguousarray(p.cts[1][:, :1]), SCALE)
    assert _err(g.decrypt_share_handles, [ct, other], 40, k1 * 2) == "ciphertext 1: limb count differs from ciphertext 0"
    other.free()
    B = g.upload_ct_batch(p.cts, SCALE)
    assert "more than 64 instances" in _err(g.decrypt_share_handles, [B, ct], 40, k1 * 65)
    g.capture_begin()
    try:
        msg = _err(g.decrypt_share_handles, [ct], 40, k1)
    finally:
        g.graph_free(g.capture_end())
    assert "cannot be captured" in msg
    bare = backend.Context(p.N, p.primes)
    try:
        assert _err(bare.decrypt_share_handles, [bare.upload_ct(p.cts[0], SCALE)], 40, k1) == "secret key not present"
    finally:
        bare.close()
    # the combination's list checks name the share
    sh = g.decrypt_share_handles([ct], 40, k1)
    out = np.zeros((1, 8))
    assert _err(g.decrypt_combine_rows, [ct], [sh, ct], 8, out) == "share 1 is not a decryption share (size 1)"
    assert _err(g.decrypt_combine_rows, [ct], [], 8, out) == "the number of parties must be 1..64"
    sh_low = g.decrypt_share_handles([low], 40, k1)
    assert _err(g.decrypt_combine_rows, [ct], [sh, sh_low], 8, out) == "share 1: limb count differs from the ciphertexts'"
    sh2 = g.decrypt_share_handles([ct, ct], 40, k1 * 2)
    assert _err(g.decrypt_combine_rows, [ct], [sh2], 8, out) == "share 0: instance count differs from the ciphertexts'"
    rescaled = g.upload_ct_batch(sh.download().reshape(1, 1, l, p.N), 2.0 * SCALE)
    assert _err(g.decrypt_combine_rows, [ct], [sh, rescaled], 8, out) == "share 1: scale differs from the ciphertexts'"
    assert "unknown output dtype" in _err(g.decrypt_combine_rows, [ct], [sh], 8, out, dtype_code=9)
    assert _err(g.decrypt_combine_rows, [ct], [sh], 0, out) == "slot count out of range"
    # the share call counts its 32 bytes per instance and brings nothing back; the context still works
    up0, down0 = g.transfer_stats()[4:6]
    sh3 = g.decrypt_share_handles([ct], 40, k1)
    up1, down1 = g.transfer_stats()[4:6]
    assert (up1 - up0, down1 - down0) == (32, 0)
    _same(sh3.download().reshape(l, p.N), p.want(l, 0, 40, fkey(1)), "after the refusals")


# ---- through the public interface: N = 4096 on [60] * 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E2E_N, E2E_BITS = 1 << 12, [60] * 4
COMMON = bytes(range(50, 82))
SIGMA = 40


def _compile(build, scale_bits, name):
    """a program without a rescale (its products stay below the waterline), so the chain is free: [60] * 4 at N = 4096"""
    prog = EvaProgram(name, vec_size=64)
    with prog:
        Output("y", build(Input("x")))
    prog.set_input_scales(scale_bits)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.prime_bits = list(E2E_BITS)
    params.poly_modulus_degree = E2E_N
    return compiled, params, sig


@pytest.fixture(scope="module")
def committee():
    """three parties with a common seed, their collective context, and a program with a rotation and a plaintext multiply"""
    compiled, params, sig = _compile(lambda x: (x << 1) * 0.5 + x, 30, "linear")
    pairs = [generate_keys(params, seed=70 + p, common_seed=COMMON) for p in range(3)]
    col = combine_public_contexts([pub for pub, _ in pairs])
    return compiled, params, sig, pairs, col


def _linear(xs):
    return np.roll(xs, -1, axis=-1) * 0.5 + xs


def _flood_bound(P, scale):
    # N P 2^sigma / scale for the flood; 1e-6 covers the encryption's noise, the encoder's rounding and the FFT's FP64 error
    return E2E_N * P * 2.0 ** SIGMA / scale + 1e-6


def test_joint_decryption_of_a_program_under_the_collective_key(committee):
    compiled, params, sig, pairs, col = committee
    xs = np.random.default_rng(0).uniform(-1, 1, 64)
    out = col.execute(compiled, col.encrypt({"x": xs.tolist()}, sig))
    kind, size, limbs, scale, _ = out.get("y")
    assert (size, limbs) == (2, len(E2E_BITS) - 1)
    col.synchronize()
    shares = []
    for pub, sec in pairs:
        sec.decrypt_share(out, SIGMA)   # (the first call creates the party's device state and uploads its key)
        before = sec.transfer_stats()
        sh = sec.decrypt_share(out, SIGMA)
        after = sec.transfer_stats()
        assert after["h2d_bytes"] - before["h2d_bytes"] == 32 and after["ct_uploads"] == before["ct_uploads"], "32 bytes per value, no value bytes"
        assert after["d2h_bytes"] == before["d2h_bytes"]
        shares.append(sh)
    got = np.array(col.combine_shares(out, shares, sig)["y"])
    diff, bound = float(np.abs(got - _linear(xs)).max()), _flood_bound(3, scale)
    print(f"joint decryption, N = {E2E_N}, {E2E_BITS}, sigma = {SIGMA}: largest slot difference {diff:.3e}, bound {bound:.3e}")
    assert 0 < diff <= bound
    assert float(np.abs(np.array(col.combine_shares(out, shares[:2], sig)["y"]) - _linear(xs)).max()) > 1.0, "two of three parties open nothing"
    # a party alone decrypts noise: nobody holds s
    assert float(np.abs(np.array(pairs[0][1].decrypt(out, sig)["y"]) - _linear(xs)).max()) > 1.0


def test_joint_decryption_of_a_batch_of_70(committee):
    compiled, params, sig, pairs, col = committee
    xs = np.random.default_rng(1).uniform(-1, 1, (70, 64))
    outs = col.execute_batch(compiled, col.encrypt_array({"x": xs}, sig, seed=2))
    assert sum(outs.segments("y")) == 70 and len(outs.segments("y")) >= 2   # the chunk boundary
    shares = [sec.decrypt_share(outs, SIGMA, seed=5 + p) for p, (_, sec) in enumerate(pairs)]
    assert all(isinstance(s, DecryptionShares) and s.batch and s.B == 70 for s in shares)
    scale = outs[0].get("y")[3]
    got = col.combine_shares(outs, shares, sig)["y"]
    assert got.shape == (70, 64) and got.dtype == np.float64
    diff, bound = float(np.abs(got - _linear(xs)).max()), _flood_bound(3, scale)
    print(f"batch of 70: largest slot difference {diff:.3e}, bound {bound:.3e}")
    assert 0 < diff <= bound
    f32 = col.combine_shares(outs, shares, sig, dtype=np.float32)["y"]
    assert np.array_equal(f32.view(np.uint32), got.astype(np.float32).view(np.uint32))
    u8 = col.combine_shares(outs, shares, sig, dtype=np.uint8)["y"]
    assert np.array_equal(u8, _u8_rule(got))
    dev = col.combine_shares(outs, shares, sig, device=True)["y"].to_numpy()
    assert np.array_equal(dev.view(np.uint64), got.view(np.uint64))
    # the single-value path on instance 69
    one = outs[69]
    sh1 = [sec.decrypt_share(one, SIGMA, seed=5 + p) for p, (_, sec) in enumerate(pairs)]
    single = np.array(col.combine_shares(one, sh1, sig)["y"])
    assert float(np.abs(single - _linear(xs[69])).max()) <= bound


def test_a_relinearizing_program_is_refused(committee):
    _, _, _, pairs, _ = committee
    compiled, params, sig = _compile(lambda x: x * x, 50, "square")
    pubs = [generate_keys(params, seed=80 + p, common_seed=COMMON)[0] for p in range(2)]
    col = combine_public_contexts(pubs)
    enc = col.encrypt({"x": [0.5] * 64}, sig)
    with pytest.raises(ValueError, match=r"relinearization key not present \(a collective context has none\)"):
        col.execute(compiled, enc)
    assert np.array(pubs[0].execute(compiled, pubs[0].encrypt({"x": [0.5] * 64}, sig)).get("y")[4]).size > 0, "an ordinary context still runs it"


def test_one_owners_result_released_to_the_committee(committee):
    """encrypt under A -> execute x^2 under A's keys -> re-key to the collective key -> joint decryption"""
    _, _, _, pairs, col = committee
    compiled, params, sig = _compile(lambda x: x * x, 50, "square")
    pub_a, sec_a = generate_keys(params, 21)
    rk = sec_a.make_rekey_key(col, seed=4)   # needs the collective PUBLIC key only
    xs = np.random.default_rng(2).uniform(-1, 1, 64)
    out_a = pub_a.execute(compiled, pub_a.encrypt({"x": xs.tolist()}, sig))
    ref = np.array(sec_a.decrypt(out_a, sig)["y"])
    handed = col.rekey(out_a, rk)
    kind, size, limbs, scale, _ = handed.get("y")
    shares = [sec.decrypt_share(handed, SIGMA) for _, sec in pairs]
    got = np.array(col.combine_shares(handed, shares, sig)["y"])
    primes = po.coeff_modulus_create(E2E_N, E2E_BITS)
    # the re-key's own bound (over the inputs' scale; the key's error is the sum of three parties') plus the flood's
    bound = 3 * rkm.slot_bound(E2E_N, primes, limbs, 50) + _flood_bound(3, scale)
    diff = float(np.abs(got - ref).max())
    print(f"A -> collective key -> joint decryption: largest slot difference {diff:.3e}, bound {bound:.3e}; against x^2 {float(np.abs(got - xs * xs).max()):.3e}")
    assert diff <= bound and bound < 0.05


_CHILD = """
import sys
sys.path.insert(0, 'tests')
from test_gpu_threshold import twin_shares
from eva import save
save(twin_shares(), sys.argv[1])
"""


def twin_shares():
    compiled, params, sig = _compile(lambda x: (x << 1) * 0.5 + x, 30, "linear")
    params.poly_modulus_degree = 1024
    params.prime_bits = [60, 30, 45, 50, 33, 60]
    pub, sec = generate_keys(params, seed=11, common_seed=COMMON)
    enc = sec.encrypt({"x": [0.25 * (i % 5) for i in range(64)]}, sig, seed=3)
    return sec.decrypt_share(enc, SIGMA, seed=9)


def test_device_share_equals_the_host_twin_child(tmp_path):
    path = str(tmp_path / "host.shares")
    child_env = dict(os.environ, PYTHONPATH=ROOT, EVA_DEVICE_CLIENT="0")
    out = subprocess.run([sys.executable, "-c", _CHILD, path], cwd=ROOT, env=child_env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    host, dev = load(path), twin_shares()
    assert isinstance(host, DecryptionShares) and (host.smudge_bits, host.names(), list(host.primes)) == (dev.smudge_bits, dev.names(), list(dev.primes))
    _same(dev.words("x")[0][0], host.words("x")[0][0], "device against the host twin")


def test_each_common_seed_pair_is_a_key_pair_of_its_own():
    """a party's own encrypt -> execute (its own Galois key: the rotation) -> decrypt round-trips, and nobody else's secret opens it.
    Inputs at scale 2^50.  Bound per slot, hard: a fresh public-key encryption has |e_pk u + e0 + e1 s| <= 21 (2 N + 1) per
    coefficient plus N + 1 from its division by the special prime, a slot sums N coefficients, and the program takes 1.5 of
    it (the rotated half and the value); the rotation's key switch adds at most rekey_model.slot_bound (the same
    sum over digits with a key error of at most 21 (2 N + 1), and its rounding)."""
    compiled, params, sig = _compile(lambda x: (x << 1) * 0.5 + x, 50, "linear50")
    pairs = [generate_keys(params, seed=90 + p, common_seed=COMMON) for p in range(3)]
    primes = po.coeff_modulus_create(E2E_N, E2E_BITS)
    bound = 1.5 * E2E_N * (21 * (2 * E2E_N + 1) + E2E_N + 1) / 2.0 ** 50 + rkm.slot_bound(E2E_N, primes, len(E2E_BITS) - 1, 50)
    assert bound < 0.01
    xs = np.random.default_rng(4).uniform(-1, 1, 64)
    for p, (pub, sec) in enumerate(pairs):
        for enc in (pub.encrypt({"x": xs.tolist()}, sig), sec.encrypt({"x": xs.tolist()}, sig, seed=1 + p)):
            out = pub.execute(compiled, enc)
            diff = float(np.abs(np.array(sec.decrypt(out, sig)["y"]) - _linear(xs)).max())
            print(f"party {p} alone: largest slot difference {diff:.3e}, bound {bound:.3e}")
            assert diff <= bound, f"party {p}"
        assert float(np.abs(np.array(pairs[(p + 1) % 3][1].decrypt(out, sig)["y"]) - _linear(xs)).max()) > 1.0


def test_no_two_values_of_a_batch_share_a_flooding_key(committee):
    """one stream SecureRng(seed, 5) per call, names sorted, instances in order: instance b of name i takes key i * B + b"""
    from eva.ckks import CKKSEncodingInfo, CKKSSignature
    from eva_amd._eva import Type
    from sampled_keys import stream_keys
    _, params, _, pairs, col = committee
    B, names, seed = 70, ["a", "b"], 13
    sig = CKKSSignature(64, {n: CKKSEncodingInfo(Type.Cipher, 30, 0) for n in names})
    xs = np.random.default_rng(6).uniform(-1, 1, (B, 64))
    vb = col.encrypt_array({"b": xs, "a": xs}, sig, seed=2)
    sec0 = pairs[0][1]
    sh = sec0.decrypt_share(vb, SIGMA, seed=seed)
    assert sh.names() == names and sh.B == B
    keys = stream_keys(seed, 5, len(names) * B)
    assert len(set(keys)) == len(keys)
    s_ntt, primes = sec0._secret_key_ntt(), list(col.primes)
    for i, name in enumerate(names):
        got = np.concatenate(sh.words(name))   # [B][l][N], the pieces in order
        assert got.shape[0] == B
        for b in (0, 1, 63, 64, 69):   # both sides of the chunk boundary
            kind, size, limbs, scale, w = vb[b].get(name)
            ct = np.asarray(w, dtype=np.uint64).reshape(2, limbs, E2E_N)
            _same(got[b], share_host(E2E_N, primes, s_ntt, ct, SIGMA, keys[i * B + b]), f"name {name}, instance {b}: key {i * B + b}")
        assert len({got[b].tobytes() for b in range(B)}) == B
    # the same seed gives the same shares, another seed others
    again = sec0.decrypt_share(vb, SIGMA, seed=seed)
    assert all(np.array_equal(np.concatenate(again.words(n)), np.concatenate(sh.words(n))) for n in names)
    assert not np.array_equal(sec0.decrypt_share(vb, SIGMA, seed=seed + 1).words("a")[0], sh.words("a")[0])
    # and a single valuation with the two names: keys 0 and 1
    one = sec0.decrypt_share(vb[5], SIGMA, seed=seed)
    for i, name in enumerate(names):
        kind, size, limbs, scale, w = vb[5].get(name)
        ct = np.asarray(w, dtype=np.uint64).reshape(2, limbs, E2E_N)
        _same(one.words(name)[0][0], share_host(E2E_N, primes, s_ntt, ct, SIGMA, keys[i]), f"single valuation, name {name}: key {i}")


def test_common_seed_keys_made_on_the_device_equal_the_host_twins(committee):
    _, params, _, _, _ = committee
    host_pub, host_sec = generate_keys(params, seed=70, common_seed=COMMON)
    dev_pub, dev_sec = generate_keys(params, seed=70, common_seed=COMMON, device_keygen=True)
    assert np.array_equal(dev_sec._secret_key_ntt(), host_sec._secret_key_ntt())
    _same(dev_pub.public_key(), host_pub.public_key(), "public key")
    hs, ds = host_pub.key_seeds(), dev_pub.key_seeds()
    assert sorted(hs) == sorted(ds) and all(np.array_equal(hs[e], ds[e]) for e in hs)
    hg, dg = host_pub.galois_keys(), dev_pub.galois_keys()
    assert sorted(hg) == sorted(dg)
    for elt in hg:
        _same(dg[elt].reshape(-1, len(E2E_BITS), E2E_N), hg[elt].reshape(-1, len(E2E_BITS), E2E_N), f"Galois key {elt}")
    _same(dev_pub.relin_key().reshape(-1, len(E2E_BITS), E2E_N), host_pub.relin_key().reshape(-1, len(E2E_BITS), E2E_N), "relinearization key")
    # a device-made party combines with host-made ones
    others = [generate_keys(params, seed=71 + p, common_seed=COMMON)[0] for p in range(2)]
    col = combine_public_contexts([dev_pub] + others)
    _same(col.public_key(), combine_public_contexts([host_pub] + others).public_key(), "collective public key")
