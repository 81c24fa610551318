"""Words that push the strided forward pass of a top-bit prime to its lazy bound, found by search.

A restatement in numpy of what the kernels compute per stage (ntt.hip.h: bfly_fwd with the top-bit reduction,
mul_tw_lazy5_add, tb_reduce_stage for the first pass), bit for bit on 64-bit words, so that the lazy value of every
element at every stage is known on the host.  The schedule lets a value grow by 4 q per unreduced stage and reduces on
every third; a butterfly actually grows its X input by t or 4 q - t, where t = Y w - q~ q in [0, 4 q) depends on the bits
of Y and w.  Constant or q - 1 polynomials never come near 4 q per stage (their lazy zeros give t = q, 2 q or 3 q), and
random ones do on one path in a few hundred.  search() draws random sub-transform inputs and keeps those on which, at a
reducing stage, X + max(t, 4 q - t) >= 2^64: the value that stage would produce if its reduction came one stage late.
On such words a reduction moved one stage down wraps a 64-bit word (for a 60-bit prime, 16 q is 2^64 less 16 c), while the
true schedule stays below 16 q.  Only the first (strided) pass on canonical input is searched: the contiguous pass and the
unreduced MAC3 rows are not."""
import os

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def shoup(w, q):
    return (int(w) << 64) // int(q)


def tb_shape(q):
    """(c, shift, mask) of q = 2^b - c, or None when q has no top-bit shape (evah_ctx_create's rule)"""
    b = int(q).bit_length()
    c = (1 << b) - int(q)
    if not (b > 32 and c < 1 << 32 and c < int(q) >> 4):
        return None
    return c, b - 32, (1 << (b - 32)) - 1


def tb_reduce_stage_first_pass(P, s):
    return s % 3 == (P - 2) % 3 or (s == 0 and (P - 2) % 3 == 2)


def _tb_reduce(X, c, sh, mask):
    hi = X >> S32
    return (hi >> np.uint64(sh)) * np.uint64(c) + (((hi & np.uint64(mask)) << S32) | (X & M32))


def _bfly(x, Y, w, ws, q):
    """X' = x + (Y w - q~ q), Y' = 2 x + 4 q - X', all mod 2^64 (mul_tw_lazy5_add)"""
    x0, x1, s0, s1 = Y & M32, Y >> S32, ws & M32, ws >> S32
    qt = x1 * s1 + ((x1 * s0) >> S32) + ((x0 * s1) >> S32)
    Xn = (x + Y * w) + qt * np.uint64((1 << 64) - q)
    return Xn, ((x << np.uint64(1)) + np.uint64((4 * q) % (1 << 64))) - Xn


def forward_stages(a, q, rp, stages, reduce_stage, late=None, trace=None, n=None):
    """`stages` Cooley-Tukey stages (twiddles rp[2^s + group], the first stages of the N-point transform) on the last axis
    of `a` (length 2^stages), lazily, with the top-bit reduction on the stages reduce_stage(s) names.  late: a list that
    receives, per reducing stage s >= 1, (s, X + max(t, 4 q - t)) as float64 — what the stage would leave unreduced;
    trace: a list that receives per stage (x, t), the X inputs after the stage's reduction and the twiddle products"""
    c, sh, mask = tb_shape(q)
    n = a.shape[-1] if n is None else n  # (stages may be fewer than log2 n: the first stages only)
    a = a.astype(np.uint64).copy()
    with np.errstate(over="ignore"):
        for s in range(stages):
            half = n >> (s + 1)
            v = a.reshape(a.shape[:-1] + (1 << s, 2, half))
            tw = np.array([int(rp[(1 << s) + g]) for g in range(1 << s)], dtype=np.uint64)
            tws = np.array([shoup(rp[(1 << s) + g], q) for g in range(1 << s)], dtype=np.uint64)
            X, Y = v[..., 0, :], v[..., 1, :]
            x = _tb_reduce(X, c, sh, mask) if reduce_stage(s) else X
            Xn, Yn = _bfly(x, Y, tw[:, None], tws[:, None], q)
            if late is not None and reduce_stage(s) and s >= 1:
                t = (Xn - x).astype(np.float64)
                late.append((s, X.astype(np.float64) + np.maximum(t, 4.0 * q - t)))
            if trace is not None:
                trace.append((x.copy(), Xn - x))
            v[..., 0, :], v[..., 1, :] = Xn, Yn
    return a


def run_start(P):
    """the first reducing stage r of the first pass whose next reducing stage is r + 3: the run on which a value may grow
    by 12 q, so that the butterfly of stage r + 3 would leave up to 17 q unreduced"""
    red = [s for s in range(P) if tb_reduce_stage_first_pass(P, s)]
    return next(r for r in red if r + 3 in red and not any(r < s < r + 3 for s in red))


def search(q_in, q, rp, P, seed=0, batch=4096, chunks=16):
    """-> an input of a 2^P-point first-pass sub-transform under prime q (twiddles rp), values below q_in, on which the
    butterfly (X index e) of reducing stage r + 3, r = run_start(P), holds X + 4 q - t >= 2^64.

    The path is the Y' output of stages r, r + 1, r + 2 above element 0: X of stage r + 3 is x_r + 12 q - (t_r + t_{r+1} +
    t_{r+2}), so it wants x_r (the reduced X input of stage r) near q and every t on it near 0, which needs the quotient
    estimate of mul_tw_lazy5 exact and Y w mod q small.  Each of the five quantities hangs on an input of its own: x_r on
    input 0, and t_s on input h_s = 2^(P - 1 - s), which reaches the Y input of the path's stage-s butterfly through X
    sides only and touches nothing else on the path.  t / q is at least the part of the quotient that the estimate's three
    dropped partial products lose, so t < d q has a probability of the order d^3: five independent scans of batch *
    chunks random values each get every t below about q / 10, which a search over whole vectors does not in 10^7 tries."""
    rng = np.random.default_rng(seed)
    red = lambda s: tb_reduce_stage_first_pass(P, s)
    r, n = run_start(P), 1 << P
    h = lambda s: n >> (s + 1)
    vec = rng.integers(0, q_in, size=n, dtype=np.uint64)

    def path_group(s):  # the path's X index at stage s is h_r + ... + h_{s-1}; its butterfly is (group, 0)
        return sum(h(u) for u in range(r, s)) >> (P - s)

    for leaf, s in [(0, r)] + [(h(s), s) for s in range(r, r + 4)]:
        g, best = path_group(s), None
        for _ in range(chunks):
            cand = np.tile(vec, (batch, 1))
            cand[1:, leaf] = rng.integers(0, q_in, size=batch - 1, dtype=np.uint64)
            trace = []
            forward_stages(cand, q, rp, s + 1, red, trace=trace, n=n)
            x, t = trace[s]
            # first scan: the largest reduced X of stage r; the others: the smallest t of stage s
            key = -x[:, g, 0].astype(np.float64) if leaf == 0 else t[:, g, 0].astype(np.float64)
            i = int(np.argmin(key))
            if best is None or key[i] < best[0]:
                best = (key[i], cand[i].copy())
        vec = best[1]
    return vec


def late_value_exact(vec, q, rp, P):
    """the largest X + max(t, 4 q - t) over the butterflies of the reducing stages s >= 1, in exact integers; also checks
    that the true schedule keeps every value below 16 q"""
    red = lambda s: tb_reduce_stage_first_pass(P, s)
    c, sh, mask = tb_shape(q)
    a = [int(x) for x in vec]
    n, best = len(a), 0
    for s in range(P):
        half = n >> (s + 1)
        for g in range(1 << s):
            w = int(rp[(1 << s) + g])
            ws = shoup(w, q)
            for j in range(half):
                i0 = g * 2 * half + j
                X, Y = a[i0], a[i0 + half]
                assert X < 16 * q and Y < 16 * q
                x = X
                if red(s):
                    hi = X >> 32
                    x = ((hi >> sh) * c + (((hi & mask) << 32) | (X & 0xFFFFFFFF)))
                x0, x1, s0, s1 = Y & 0xFFFFFFFF, Y >> 32, ws & 0xFFFFFFFF, ws >> 32
                qt = (x1 * s1 + ((x1 * s0) >> 32) + ((x0 * s1) >> 32)) % (1 << 64)
                t = (Y * w - qt * q) % (1 << 64)
                assert t < 4 * q
                if red(s) and s >= 1:
                    best = max(best, X + max(t, 4 * q - t))
                a[i0], a[i0 + half] = x + t, x + 4 * q - t
    return best


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LOG_DEGREES = [10, 11, 13, 14, 15, 16, 17]  # 2^12 has the pass size of 2^11
DIGIT, OUTPUT = 0, 1  # the stored inputs are digits of limb 0 transformed under prime 1 of coeff_modulus_create(N, [60] * 4)


def stored_vectors(N):
    """the inputs search() found for degree N (python tests/lazy_bound_words.py writes them; test_lazy_bound_words.py
    checks each in exact arithmetic against the primes and twiddles of today)"""
    return np.load(os.path.join(GOLDEN, f"lazy_bound_words_N{N}.npy"))


def bound_reaching_poly(N):
    """coefficients of a polynomial whose every strided-pass column holds one of stored_vectors(N)"""
    vecs = stored_vectors(N)
    cols = N // vecs.shape[1]
    coeff = np.empty(N, dtype=np.uint64)
    for col in range(cols):  # sub-transform element e of column col is coefficient col + e * cols
        coeff[col::cols] = vecs[col % len(vecs)]
    return coeff


if __name__ == "__main__":
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import pyoracle as po

    for logN in [int(a) for a in sys.argv[1:]] or LOG_DEGREES:
        N, P = 1 << logN, (logN + 1) // 2
        primes = po.coeff_modulus_create(N, [60] * 4)
        rp = po.Oracle(N, primes).root_powers(OUTPUT)
        vecs, late = [], []
        for i in range(12):  # the margin depends on the twiddles' low words: keep the inputs that make it, up to four
            v = search(primes[DIGIT], primes[OUTPUT], rp, P, seed=100 * logN + i)
            x = late_value_exact(v, primes[OUTPUT], rp, P)
            if x >= 1 << 64:
                vecs.append(v)
                late.append(x)
            if len(vecs) == 4:
                break
        print(f"N=2^{logN} P={P} run from stage {run_start(P)}: late values / 2^64 =", [round(x / 2.0 ** 64, 5) for x in late], flush=True)
        assert vecs
        np.save(os.path.join(GOLDEN, f"lazy_bound_words_N{N}.npy"), np.stack(vecs))
