"""The arithmetic primitives the kernels are built on (devmath.hip.h, the butterflies of ntt.hip.h, the key-switch
accumulators of ntt_ks_inner.hip.h), run on the GPU through evah_test_devmath and checked against exact Python integers:
both the value (congruent, or canonical where canonical is promised) and the range each lazy bound claims.  The words
sit at the edges of each precondition (0, q - 1, kq - 1, 2^32, 2^60 - 1, 2^64 - 1, a low word that carries), the
sequences run to exactly the stated maximum number of maximal terms, and where a limit is a real edge one case just
past it shows that the limit is needed."""
import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
M30 = (1 << 30) - 1
WIDTHS = [20, 30, 31, 32, 33, 34, 40, 50, 53, 54, 55, 59, 60]


def _is_prime(n):
    return po.lib.evo_is_prime(n)


def _ntt_prime_below(bound, N):
    q = bound - (bound % (2 * N)) + 1
    while q >= bound or not _is_prime(q):
        q -= 2 * N
    return q


def _create(N, bits):
    try:
        return po.coeff_modulus_create(N, [bits])[0]
    except Exception:
        return None  # no prime of that width for this N


def _ctx_sets():
    """(name, N, primes): every prime is exercised with the DevPrime its context builds."""
    sets = []
    for N in (1024, 131072):
        ps = [q for q in (_create(N, b) for b in WIDTHS) if q is not None]
        sets.append((f"create_N{N}", N, ps))
    N = 1024
    # not of the top-bit shape: c = 2^b - q >= 2^32
    below54 = _ntt_prime_below((1 << 54) - (1 << 36), N)
    nontb55 = _ntt_prime_below((1 << 55) - (1 << 40), N)
    nontb56 = _ntt_prime_below((1 << 56) - (1 << 40), N)
    # c on both sides of q / 16 (b = 36: c ~ 2^31.9 < 2^32), and far below 2^33 / 2^34 (c close to 2^32, c > q / 16)
    q16 = (1 << 36) * 16 // 17
    sets.append(("below54", N, [below54, _create(N, 60)]))
    sets.append(("nontb55", N, [nontb55, _create(N, 60)]))
    sets.append(("nontb56", N, [nontb56, _create(N, 60)]))
    sets.append(("c_q16", N, [_ntt_prime_below(q16 + (1 << 28), N), _ntt_prime_below(q16 - (1 << 28), N),
                              _ntt_prime_below(int(1.2 * 2 ** 32), N), _ntt_prime_below(int(3.05 * 2 ** 32), N)]))
    # a 60-bit prime of the top-bit shape with c just above 2^31 (CoeffModulus::Create's have c < 2^30): its digits
    # reach 2^60 + 28 * 2^30, the largest radix-2^30 products
    sets.append(("bigc60", N, [_ntt_prime_below((1 << 60) - (1 << 31), N), _create(N, 60)]))
    return sets


SETS = _ctx_sets()
_CTX = {}


def _ctx(name):
    if name not in _CTX:
        _, N, ps = next(s for s in SETS if s[0] == name)
        _CTX[name] = backend.Context(N, ps)
    return _CTX[name], next(s for s in SETS if s[0] == name)[2]


def _shape(q):
    """(b, c, top-bit shape?) as runtime.hip decides it"""
    b = q.bit_length()
    c = (1 << b) - q
    return b, c, b > 32 and c < (1 << 32) and c < (q >> 4)


def _edges(q, limit=M64):
    w = [0, 1, q - 1, q, 2 * q - 1, 4 * q - 1, 8 * q - 1, 12 * q - 1, 16 * q - 1, (1 << 32) - 1, 1 << 32,
         (1 << 60) - 1, M64, M64 - q, (1 << 63)]
    return sorted({x for x in w if 0 <= x <= limit})


def _rand(rng, n, hi):
    return [int(x) for x in rng.integers(0, hi, size=n, dtype=np.uint64)] if hi <= M64 else \
        [int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4)) for _ in range(n)]


def _arr(v):
    return np.array([int(x) & M64 for x in v], dtype=np.uint64)


def _shoup(w, q):
    return (w << 64) // q


def _run(g, pi, op, a, b=None, c=None):
    a = np.array(a, dtype=np.uint64) if not isinstance(a, np.ndarray) else a
    out = g.test_devmath(pi, op, a, None if b is None else np.array(b, dtype=np.uint64),
                         None if c is None else np.array(c, dtype=np.uint64))
    return [int(x) for x in out[:, 0]], [int(x) for x in out[:, 1]]


def _pairs(q, rng, xs_limit=M64):
    """(x, w) over the edge words x and twiddles w in {0, 1, q - 1, random}, plus random pairs"""
    ws = [0, 1, q - 1, q >> 1] + _rand(rng, 3, q)
    xs = _edges(q, xs_limit) + _rand(rng, 16, min(xs_limit, M64) + 1 if xs_limit < M64 else M64)
    P = [(x, w) for x in xs for w in ws]
    P += list(zip(_rand(rng, 2000, M64), _rand(rng, 2000, q)))
    return P


ALL_PRIMES = [(name, i, q) for name, _, ps in SETS for i, q in enumerate(ps)]


@pytest.mark.parametrize("name,pi,q", ALL_PRIMES, ids=lambda v: str(v))
def test_modular_products_and_reductions(name, pi, q):
    g, _ = _ctx(name)
    rng = np.random.default_rng(q % 1000003)
    P = _pairs(q, rng)
    xs, ws = [x for x, _ in P], [w for _, w in P]
    wss = [_shoup(w, q) for w in ws]
    c = [[s, 0] for s in wss]
    # mul_shoup_lazy: x w mod q in [0, 2q) for ANY 64-bit x; mul_shoup canonical
    r, _ = _run(g, pi, "mul_shoup_lazy", _arr(xs), _arr(ws), c)
    for x, w, v in zip(xs, ws, r):
        assert v % q == x * w % q and v < 2 * q, (hex(x), hex(w), hex(v))
    r, _ = _run(g, pi, "mul_shoup", _arr(xs), _arr(ws), c)
    assert r == [x * w % q for x, w in zip(xs, ws)]
    # mul_tw_lazy5: congruent, < 4q for ANY 64-bit x
    r, _ = _run(g, pi, "mul_tw_lazy5", _arr(xs), _arr(ws), c)
    for x, w, v in zip(xs, ws, r):
        assert v % q == x * w % q and v < 4 * q, (hex(x), hex(w), hex(v))
    # the butterflies' form: a + (x w - q~ q), the mad chain started from a; both forms give the same word
    adds = [[0, 1, q - 1, 8 * q - 1, 12 * q - 1][i % 5] for i in range(len(xs))]
    c2 = [[s, a] for s, a in zip(wss, adds)]
    r1, _ = _run(g, pi, "mul_tw_lazy5_add", _arr(xs), _arr(ws), c2)
    r2, _ = _run(g, pi, "mul_tw_lazy5_add_mad", _arr(xs), _arr(ws), c2)
    assert r1 == r2
    for x, w, a, v in zip(xs, ws, adds, r1):
        assert a <= v < a + 4 * q and (v - a) % q == x * w % q, (hex(x), hex(w), hex(a), hex(v))
    # barrett64: canonical for any 64-bit x
    r, _ = _run(g, pi, "barrett64", _arr(xs))
    assert r == [x % q for x in xs]


@pytest.mark.parametrize("name,pi,q", ALL_PRIMES, ids=lambda v: str(v))
def test_128bit_reductions(name, pi, q):
    """barrett128 canonical and reduce128_lazy congruent for ANY (hi, lo); lo near 2^64 makes t + lo carry, the case
    its one fix-up with 2^64 mod q is there for"""
    g, _ = _ctx(name)
    rng = np.random.default_rng(q % 999983)
    his = [0, 1, q - 1, q, (1 << 32) - 1, 1 << 32, (1 << 60) - 1, M64, M64 - 1] + _rand(rng, 6, M64)
    los = [0, 1, q - 1, M64, M64 - 1, M64 - q, M64 - 4 * q + 1, (1 << 63)] + _rand(rng, 4, M64)
    X = [(h, lo) for h in his for lo in los] + list(zip(_rand(rng, 3000, M64), _rand(rng, 3000, M64)))
    lo, hi = _arr([x[1] for x in X]), _arr([x[0] for x in X])
    r, _ = _run(g, pi, "barrett128", lo, hi)
    exp = [((h << 64) | l) % q for h, l in X]
    bad = [(hex(h), hex(l)) for (h, l), v, e in zip(X, r, exp) if v != e]
    assert not bad, f"{len(bad)} wrong, e.g. {bad[:3]}"
    r, _ = _run(g, pi, "reduce128_lazy", lo, hi)
    assert all(v % q == e for v, e in zip(r, exp))


@pytest.mark.parametrize("name,pi,q", ALL_PRIMES, ids=lambda v: str(v))
def test_add_sub_neg_and_top_bit_reduction(name, pi, q):
    g, _ = _ctx(name)
    rng = np.random.default_rng(q % 99991)
    can = [0, 1, q - 1, q >> 1, (q >> 1) + 1] + _rand(rng, 500, q)
    A = [(a, b) for a in can[:5] for b in can[:5]] + list(zip(can, can[::-1]))
    a, b = _arr([x for x, _ in A]), _arr([y for _, y in A])
    assert _run(g, pi, "addmod", a, b)[0] == [(x + y) % q for x, y in A]
    assert _run(g, pi, "submod", a, b)[0] == [(x - y) % q for x, y in A]
    assert _run(g, pi, "negmod", a)[0] == [(-x) % q for x, _ in A]
    # top-bit reduction x -> (x mod 2^b) + (x >> b) c: congruent; < q + 16c for x < 16q; < 2^b + (2^(64-b) - 1) c for
    # any x (< 2^60 + 2^36 at b = 60); the identity for a prime of another shape
    bq, cq, tb = _shape(q)
    xs = _edges(q) + _rand(rng, 2000, M64) + [(1 << bq) - 1 + (k << bq) for k in range(min(64, 1 << (64 - bq)))]
    xs = [x for x in xs if x <= M64]
    r, _ = _run(g, pi, "topbit", _arr(xs))
    for x, v in zip(xs, r):
        if not tb:
            assert v == x
            continue
        assert v % q == x % q, (hex(x), hex(v))
        assert v < (1 << bq) + ((M64 >> bq) * cq)
        if x < 16 * q:
            assert v < q + 16 * cq, (hex(x), hex(v))
        if bq <= 60:
            assert v < (1 << 60) + (1 << 36)


def test_top_bit_shape_is_chosen_only_where_its_bound_holds():
    """runtime.hip: the top-bit butterflies need x < q + 16c after the reduction and three lazy stages (+ 12q) on top
    of it to stay below 16q: 16c < 3q.  The shape test asks c < 2^32 and c < q / 16; a prime of 2^b - c with c close to
    2^32 (far below 2^33 or 2^34) must not get it, primes with c just under q / 16 do."""
    seen = {True: 0, False: 0}
    for name, pi, q in ALL_PRIMES:
        g, _ = _ctx(name)
        b, c, tb = _shape(q)
        v, _ = _run(g, pi, "topbit", _arr([1 << b]) if b < 64 else _arr([0]))
        active = v[0] != (1 << b)
        assert active == tb, (name, hex(q))
        if active:
            assert q + 16 * c + 12 * q < 16 * q, (name, hex(q))
        seen[active] += 1
    assert seen[True] and seen[False]
    # both sides of q / 16 are in the set
    qs = _ctx("c_q16")[1]
    assert [_shape(q)[2] for q in qs] == [True, False, False, False]


@pytest.mark.parametrize("name,pi,q", ALL_PRIMES, ids=lambda v: str(v))
def test_butterflies(name, pi, q):
    """bfly_fwd<REDUCE, MAD, TB>: X < 16q (REDUCE) / < 12q (plain), any Y -> X' = x + t, Y' = x + 4q - t with t = Y w mod q
    lazy in [0, 4q): outputs < 12q / < 16q (the TB reduction: x < q + 16c).  bfly_inv: X, Y < 5q -> X + Y folded below
    5q and (X - Y) w lazy below 4q."""
    g, _ = _ctx(name)
    rng = np.random.default_rng(q % 65537)
    b, c, tb = _shape(q)
    ws = [1, q - 1] + _rand(rng, 2, q)
    for red in (0, 1):
        Xmax = 16 * q if red else 12 * q
        Xs = [0, 1, q - 1, q, 4 * q - 1, 8 * q - 1, 8 * q, Xmax - 1] + _rand(rng, 300, Xmax)
        Ys = [0, q - 1, 16 * q - 1, M64] + _rand(rng, 300, M64)
        T = [(x, y, w) for x in Xs[:8] for y in Ys[:4] for w in ws] + list(zip(Xs, Ys, _rand(rng, 308, q)))
        X, Y, W = _arr([t[0] for t in T]), _arr([t[1] for t in T]), [t[2] for t in T]
        cw = [[w, _shoup(w, q)] for w in W]
        for mad in (0, 1):
            for tbf in (0, 1):
                if tbf and not tb and red:
                    continue  # the passes never reduce a prime of another shape with the top-bit form
                x1, y1 = _run(g, pi, f"bfly_fwd_{red}{mad}{tbf}", X, Y, cw)
                for (x, y, w), u, v in zip(T, x1, y1):
                    xr = x
                    if red and tbf:
                        xr = (x & ((1 << b) - 1)) + (x >> b) * c
                        assert xr < q + 16 * c
                    elif red:
                        xr = x - 8 * q if x >= 8 * q else x
                    t = u - xr
                    assert 0 <= t < 4 * q and t % q == y * w % q, (red, mad, tbf, hex(x), hex(y), hex(w), hex(u))
                    assert v == xr + 4 * q - t
                    lim = (q + 16 * c + 8 * q) if (red and tbf) else (12 * q if red else 16 * q)
                    assert u < lim and v < lim
    Xs = [0, 1, q - 1, q, 5 * q - 1] + _rand(rng, 400, 5 * q)
    T = [(x, y, w) for x in Xs[:5] for y in Xs[:5] for w in ws] + list(zip(Xs, Xs[::-1], _rand(rng, 405, q)))
    cw = [[w, _shoup(w, q)] for _, _, w in T]
    x1, y1 = _run(g, pi, "bfly_inv", _arr([t[0] for t in T]), _arr([t[1] for t in T]), cw)
    for (x, y, w), u, v in zip(T, x1, y1):
        assert u < 5 * q and u % q == (x + y) % q
        assert v < 4 * q and v % q == (x - y) * w % q


@pytest.mark.parametrize("name,pi,q", ALL_PRIMES, ids=lambda v: str(v))
def test_acc128_and_acc128c_exact(name, pi, q):
    """acc128 is exact 128-bit arithmetic.  acc128c (operands < 2^60) is exact while the sum stays below 2^128: up to
    256 maximal products; accumulators whose low word is near 2^64 force the carry out of its first v_mad_u64_u32."""
    g, _ = _ctx(name)
    rng = np.random.default_rng(q % 7919)
    top = min(q, 1 << 60)
    m = 256
    cases = []  # (init lo, init hi, a terms, b terms)
    ext = [top - 1, (1 << 60) - 1, q - 1]
    for e in ext:
        cases.append((0, 0, [e] * m, [e] * m))
    for lo in (M64, M64 - 1, M64 - (1 << 32), 1 << 63):
        cases.append((lo, 0, [top - 1] * m, [top - 1] * m))
        cases.append((lo, 5, _rand(rng, m, top), _rand(rng, m, top)))
        cases.append((lo, 0, [(1 << 32) - 1] * m, [(1 << 32) - 1] * m))
        cases.append((lo, 0, [1 << 32] * m, [(1 << 32) - 1] * m))
    for _ in range(64):
        cases.append((int(rng.integers(0, 1 << 63)) * 2 + 1, int(rng.integers(0, 1 << 20)),
                      _rand(rng, m, top), _rand(rng, m, top)))
    A = np.array([[x & M64 for x in cs[2]] for cs in cases], dtype=np.uint64)
    B = np.array([[x & M64 for x in cs[3]] for cs in cases], dtype=np.uint64)
    C = [[cs[0], cs[1]] for cs in cases]
    exact = [(cs[0] + (cs[1] << 64) + sum(a * b for a, b in zip(cs[2], cs[3]))) for cs in cases]
    for op in ("acc128", "acc128c"):
        lo, hi = _run(g, pi, op, A, B, C)
        for e, l, h in zip(exact, lo, hi):
            if e < (1 << 128):
                assert (h << 64) | l == e, (op, hex(e), hex(h), hex(l))
            elif op == "acc128":
                assert (h << 64) | l == e % (1 << 128)


def _mac3_exact(g, pi, digits, keys, period=0):
    A = np.array([[d & M64 for d in row] for row in digits], dtype=np.uint64)
    B = np.array([[(k & M30) | ((k >> 30) << 32) for k in row] for row in keys], dtype=np.uint64)
    lo, hi = _run(g, pi, "mac3", A, B, [[period, 0]] * len(digits))
    return [(h << 64) | l for l, h in zip(lo, hi)]


def test_mac3_sums_at_their_documented_limits():
    """The radix-2^30 sums on their own (a prime below 2^54 without the top-bit shape, where the digit reduction is the
    identity): digits below 2^60 + 2^36, key halves below 2^30.  Fifteen digits (the l <= 15 gate) of maximal words are
    exact with the fold every MAC3_FOLD_DIGITS = 7.  Past the limits: 8 digits without a fold overflow the middle sum,
    16 digits overflow the top sum, which is never folded."""
    g, ps = _ctx("below54")
    assert not _shape(ps[0])[2]
    vmax, kmax = (1 << 60) + (1 << 36) - 1, (1 << 60) - 1
    v1max = ((1 << 60) + (1 << 36) - (1 << 30)) | M30  # v0 = 2^30 - 1 and the largest v1
    rng = np.random.default_rng(3)
    rows, keys, exp = [], [], []
    for m in range(1, 16):
        for d, k in ((vmax, kmax), (v1max, kmax), (v1max, (M30 << 30) | M30)):
            rows.append([d] * m)
            keys.append([k] * m)
            exp.append(m * d * k)
        ds, ks = _rand(rng, m, vmax + 1), _rand(rng, m, kmax + 1)
        rows.append(ds)
        keys.append(ks)
        exp.append(sum(a * b for a, b in zip(ds, ks)))
    assert _mac3_row_by_row(g, rows, keys) == exp
    # past the limits
    assert _mac3_exact(g, 0, [[v1max] * 8], [[kmax] * 8], period=8)[0] != 8 * v1max * kmax
    assert _mac3_exact(g, 0, [[v1max] * 16], [[kmax] * 16])[0] != 16 * v1max * kmax


def _mac3_row_by_row(g, rows, keys):
    """MAC3 sums of sequences of different lengths (one call per length)"""
    by_len, res = {}, [None] * len(rows)
    for i, r in enumerate(rows):
        by_len.setdefault(len(r), []).append(i)
    for idx in by_len.values():
        for i, v in zip(idx, _mac3_exact(g, 0, [rows[i] for i in idx], [keys[i] for i in idx])):
            res[i] = v
    return res


def _worst_digits(q):
    """Digit words x < 16q whose top-bit reduction v = v0 + v1 2^30 maximises v0 k1 + v1 k0 (the middle sum)"""
    b, c, tb = _shape(q)
    if not tb:
        return [41 * q - 1, 16 * q - 1, q - 1]
    out = {16 * q - 1, q - 1, (1 << b) - 1}
    for h in range(1, 16):
        base = (h << b)
        top = min((1 << b) - 1, 16 * q - 1 - base)
        if top < 0:
            continue
        # the largest x mod 2^b that makes v's low 30 bits all ones
        v = top + h * c
        v = v - ((v - M30) % (1 << 30))
        if v - h * c >= 0:
            out.add(base + v - h * c)
        out.add(base + top)
    return sorted(out)


def _worst_keys(q):
    k = q - 1
    ks = {k, ((k >> 30) << 30) - 1 if k >= (1 << 30) else k, min(k, M30)}
    if (k >> 30) > 0:
        ks.add((((k >> 30) - 1) << 30) | M30)  # k0 = 2^30 - 1 under the largest k1 it allows
    return sorted(x for x in ks if 0 <= x < q)


@pytest.mark.parametrize("name,pi,q", ALL_PRIMES, ids=lambda v: str(v))
def test_mac3_exact_on_each_prime(name, pi, q):
    """ks_inner_kernel<MAC3>'s accumulation on the prime's own DevPrime: the worst digits of the transforms' range
    (< 16q through the top-bit reduction; < 41q unreduced for a prime of another shape below 2^54) times key words up to
    q - 1, 1..15 digits, must give the exact sum of v * k.  A context that contains a prime of another shape at or above
    2^54 must not use MAC3 at all."""
    g, ps = _ctx(name)
    b, c, tb = _shape(q)
    eligible = all(_shape(p)[2] or p < (1 << 54) for p in ps)
    if not eligible:
        with pytest.raises(backend.EvaHipError):
            _mac3_exact(g, pi, [[1]], [[1]])
        return
    red = (lambda x: (x & ((1 << b) - 1)) + (x >> b) * c) if tb else (lambda x: x)
    digits, keys = _worst_digits(q), _worst_keys(q)
    for m in (1, 7, 8, 14, 15):
        rows = [[d] * m for d in digits for _ in keys]
        krs = [[k] * m for _ in digits for k in keys]
        got = _mac3_exact(g, pi, rows, krs)
        for r, kr, v in zip(rows, krs, got):
            assert v == sum(red(d) * k for d, k in zip(r, kr)), (m, hex(r[0]), hex(kr[0]), hex(v))


def test_contexts_that_may_use_mac3():
    """MAC3 applies when every prime has the top-bit shape or lies below 2^54 (runtime.hip): a 55- or 56-bit prime of
    another shape takes the 128-bit path.  The reason: such a row runs MAC3 unreduced (< 41q), and 41q must stay below
    2^60 for the split at bit 30 — at 56 bits seven maximal digits already overflow the middle sum."""
    for name, expect in (("below54", True), ("nontb55", False), ("nontb56", False), ("create_N1024", True)):
        g, ps = _ctx(name)
        try:
            _mac3_exact(g, 0, [[1]], [[1]])
            ok = True
        except backend.EvaHipError:
            ok = False
        assert ok == expect, name
    q = _ctx("nontb56")[1][0]
    v, k = 41 * q - 1, q - 1
    v0, v1, k0, k1 = v & M30, v >> 30, k & M30, k >> 30
    assert 7 * (v0 * k1 + v1 * k0) >= 1 << 64  # what the middle sum would have to hold


@pytest.mark.parametrize("name,pi,q", ALL_PRIMES, ids=lambda v: str(v))
def test_128bit_key_switch_accumulation(name, pi, q):
    """The non-MAC3 inner product: lazy digits < 16q times key words < q, folded to one word every KS128_FOLD_DIGITS =
    15, then the three P d_K terms of the fold modes (a canonical word times a lazy one < 4q).  Exact modulo q at
    l = 1..31 with maximal words.  Past the limit: 16 maximal digits and the three terms overflow 128 bits at 60 bits."""
    g, _ = _ctx(name)
    dmax, kmax, a, u = 16 * q - 1, q - 1, q - 1, 4 * q - 1
    rng = np.random.default_rng(q % 4099)
    for m in (1, 15, 16, 17, 30, 31):
        rows = [[dmax] * m, [dmax] * (m - 1) + [0], _rand(rng, m, 16 * q)]
        krs = [[kmax] * m, [kmax] * m, _rand(rng, m, q)]
        lo, hi = _run(g, pi, "ks128", np.array(rows, dtype=np.uint64), np.array(krs, dtype=np.uint64), [[a, u]] * 3)
        for r, kr, l, h in zip(rows, krs, lo, hi):
            assert ((h << 64) | l) % q == (sum(x * y for x, y in zip(r, kr)) + 3 * a * u) % q, (m, hex(q))
    if q.bit_length() == 60:
        assert 16 * dmax * kmax + 3 * a * u >= 1 << 128
