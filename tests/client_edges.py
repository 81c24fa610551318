"""Case builders shared by test_gpu_client_edges.py and test_client_edges_cpu.py: the inputs that take the client
kernels to their arithmetic edges, and the expectations that need nothing but Python integers and rationals.

  dense_values      two dense value vectors for the special FFT (no slot zero, magnitudes over nine decades)
  edge_values       composed coefficients x in [0, Q) on the sign decision, on the word boundaries and on the mixed
                    per-word signs of the recomposition (crt_to_double, the oracle's evo_decode, the host decoder)
  constant_cts      ciphertexts of the constant polynomials x_b; poly_ct: of one polynomial with chosen coefficients
  b1_bound          the derived error bound of the recomposition of one coefficient
  encoder_cases     integers m for the encoder's rounding: a constant vector m / scale encodes to the constant m
  device_accepts    the refusal rule of the device encoder, restated"""
import math
from fractions import Fraction

import numpy as np

W = 1 << 64

# (N, prime bits, scale bits): every chain is decoded at l = len(bits) - 1, its deepest level
RECOMP_CHAINS = [
    (1024, [50, 60], 30),                 # l = 1: Q in one word
    (1024, [60, 60, 60, 60], 30),         # l = 3: three words
    (1024, [40, 30, 40, 41], 30),         # l = 3, Q in two words: the top word of Q and of floor(Q/2) is 0
    (4096, [40] * 19 + [41], 30),         # l = 19
    (1024, [60] * 17, 30),                # l = 16
    (1024, [30] * 62, 900),               # l = 61, the deepest the call accepts; 2^900 keeps Q / scale a finite double
]


def chain_id(cfg):
    return f"N{cfg[0]}-l{len(cfg[1]) - 1}-{cfg[1][0]}bit"


def product(primes):
    Q = 1
    for q in primes:
        Q *= int(q)
    return Q


def words_of(x, n):
    return [(x >> (64 * w)) & (W - 1) for w in range(n)]


def word_count(Q):
    return (Q.bit_length() + 63) // 64


def centered(x, Q):
    """the signed value the decoders give x: negative above floor(Q/2)"""
    return x - Q if x > Q // 2 else x


def dense_values(rng, n):
    """[2][n]: uniform in (-4, 4), and random signs times 10^u with u uniform in [-6, 3] — with magnitudes over nine
    decades an FP64 reordering or a wrong root shows in the low bits of the result"""
    uniform = rng.uniform(-4, 4, n)
    mixed = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, 3, n)
    return np.stack([uniform, mixed])


def edge_values(primes, rng, multiple=64):
    """distinct x in [0, Q), Q = the product of `primes`, h = floor(Q/2): the named edges first, then random fillers up to
    the next multiple of `multiple` values"""
    Q = product(primes)
    h, nw = Q // 2, word_count(Q)
    qw = words_of(Q, nw)
    xs = [0, 1, Q - 1, h - 1, h, h + 1, h + 2]
    for w in range(nw):                      # a word boundary of x from below and above
        xs += [(1 << 64 * w) - 1, 1 << 64 * w, (1 << 64 * w) + 1]
    for w in range(nw):                      # the same distance below Q: the negative branch's boundaries
        xs += [Q - (1 << 64 * w) - 1, Q - (1 << 64 * w), Q - (1 << 64 * w) + 1]
    if nw > 1:
        xs.append(Q - (Q % W) - 1)           # word 0 exceeds Q's, word 1 falls short of it
    for p in range(nw - 1):                  # words 0 .. p exceed Q's, the top word falls short: mixed per-word signs
        for low in (lambda w: min(qw[w] + 1, W - 1), lambda w: W - 1):
            ws = [low(w) if w <= p else qw[w] for w in range(nw)]
            ws[nw - 1] = qw[nw - 1] - 1 if qw[nw - 1] else 0
            xs.append(sum(v << 64 * w for w, v in enumerate(ws)))
    out = []
    for x in xs:
        x %= Q
        if x not in out:
            out.append(x)
    while len(out) % multiple:
        x = int.from_bytes(rng.bytes((Q.bit_length() + 7) // 8 + 8), "little") % Q
        if x not in out:
            out.append(x)
    return out


def recomp_cases(primes_of):
    """(chain, chunk) for every 64 edge values of every chain of RECOMP_CHAINS — one decrypt_decode_many call each;
    primes_of(N, bits) = the chain's primes"""
    out = []
    for cfg in RECOMP_CHAINS:
        l = len(cfg[1]) - 1
        n = len(edge_values(primes_of(cfg[0], cfg[1])[:l], np.random.default_rng(l)))
        out += [(cfg, c) for c in range(n // 64)]
    return out


def case_id(case):
    return f"{chain_id(case[0])}-{case[1]}"


def accumulated_words(x, primes):
    """the signed words d_w the recomposition turns into doubles: x's words, or x_w - Q_w in the negative branch"""
    Q = product(primes)
    n = len(primes)   # `limbs` words per coefficient, the high ones zero
    xw, qw = words_of(x, n), words_of(Q, n)
    return [a - b for a, b in zip(xw, qw)] if x > Q // 2 else xw


def b1_bound(x, primes, scale):
    """A bound on |double the recomposition returns - centered(x) / scale|, as a Fraction.
    The algorithm sums, least significant word first, fl(d_w) * (2^(64 w) / scale) over the l words d_w of
    accumulated_words, whose exact sum is centered(x).  With scale a power of two every factor 2^(64 w) / scale is a
    power of two, so the product is exact and the rounding errors are: one per conversion of a 64-bit word to a double
    (relative 2^-53) and one per addition (relative 2^-53 of a partial sum, itself at most S / scale (1 + l 2^-53) with
    S = sum |d_w| 2^(64 w)).  l conversions and at most l additions give |error| <= ((1 + 2^-53)^(l + 1) - 1) S / scale
    < 2 (l + 1) 2^-53 S / scale.  Nothing in it is measured."""
    l = len(primes)
    S = sum(abs(d) << 64 * w for w, d in enumerate(accumulated_words(x, primes)))
    return Fraction(2 * (l + 1) * S, 1 << 53) / Fraction(scale)


def check_constant_decodes(xs, rows, primes, scale, what):
    """rows[b]: the decoded slots of the constant polynomial xs[b].  Every slot carries the same double (the special FFT
    of a delta at coefficient 0 only adds +-0 to it), that double is within b1_bound of the exact rational
    centered(x) / scale, and it has the sign of centered(x)."""
    Q = product(primes)
    for x, row in zip(xs, rows):
        row = np.asarray(row, dtype=np.float64)
        assert np.all(row.view(np.uint64) == row.view(np.uint64)[0]), f"{what}: x = {x:#x}: the slots differ"
        exact = Fraction(centered(x, Q)) / Fraction(scale)
        err, bound = abs(Fraction(float(row[0])) - exact), b1_bound(x, primes, scale)
        assert err <= bound, f"{what}: x = {x:#x}: error {float(err):.3g} above the bound {float(bound):.3g}"
        if abs(exact) > bound:
            assert (row[0] > 0) == (exact > 0), f"{what}: x = {x:#x}: sign"


def ternary_key(o, rng):
    """a ternary secret under every prime of the oracle's chain, NTT form [k][N]"""
    s = rng.integers(-1, 2, size=o.N)
    return np.stack([o.ntt(i, np.array([int(v) % q for v in s], dtype=np.uint64)) for i, q in enumerate(o.primes)])


def hide(o, l, sk, m_ntt, rng):
    """a size-2 ciphertext of the NTT-form message m_ntt [l][N]: c0 = m - c1 s with uniformly random c1"""
    q = np.array(o.primes[:l], dtype=np.uint64)[:, None]
    c1 = rng.integers(0, q, size=(l, o.N), dtype=np.uint64)
    rest = o.decrypt(np.stack([np.zeros_like(c1), c1]), sk)          # c1 s
    return np.stack([(m_ntt + q - rest) % q, c1])                     # every term below 2^62: no wrap


def constant_cts(o, l, sk, xs, rng):
    """one ciphertext per x of the constant polynomial x: its NTT form is x mod q_i in every slot"""
    out = []
    for x in xs:
        m = np.array([[x % q] for q in o.primes[:l]], dtype=np.uint64) * np.ones((1, o.N), dtype=np.uint64)
        out.append(hide(o, l, sk, m, rng))
    return out


def poly_ct(o, l, sk, coeffs, rng):
    """a ciphertext of the polynomial with the integer coefficients `coeffs` (N values in [0, Q))"""
    m = np.stack([o.ntt(i, np.array([x % q for x in coeffs], dtype=np.uint64)) for i, q in enumerate(o.primes[:l])])
    return hide(o, l, sk, m, rng)


def cycled(xs, N):
    return [xs[j % len(xs)] for j in range(N)]


# ---- the encoder's rounding

# (N, prime bits): the encoder's chains, at scale 2^30 and l = len(bits) - 1
ENCODER_CHAINS = [(4096, [60, 30, 60, 60]), (1024, [40, 30, 40, 41])]
ENC_SCALE_BITS = 30


def encoder_cases(primes):
    """integers m of at most 53 significant bits and |m| < 2^62, so that m / 2^30 is a double and the constant vector
    m / scale encodes exactly to the constant polynomial m (the inverse special FFT of a constant only doubles, forms
    differences that are +-0 and multiplies by a power of two): the expected NTT-form plaintext is m mod q_i in every
    slot.  The list: 0; +-1; the rounding threshold 2^52 from both sides and the last odd double 2^53 - 1; odd * 2^t up
    to the documented limit 2^62 - 2^9; and for every prime q of the chain that a double holds, +-q and +-q 2^t, whose
    residue under q is 0 and must not become q for the negative sign."""
    ms = [0, 1, (1 << 52) - 1, 1 << 52, (1 << 52) + 1, (1 << 53) - 1]
    ms += [((1 << 53) - 1) << t for t in (3, 6, 7, 9)] + [3 << 60, 5 << 57, ((1 << 40) + 1) << 15]
    for q in primes:
        if q.bit_length() <= 53:
            top = 61 - q.bit_length()
            ms += [q << t for t in sorted({0, 1, 20, top - 2, top}) if (q << t) < (1 << 62) - (1 << 9)]
    out = []
    for m in ms:
        for s in (m, -m):
            if s not in out:
                out.append(s)
    assert all(abs(m) <= (1 << 62) - (1 << 9) and float(m) == m for m in out)
    return out


def constant_plaintext(m, primes, l, N):
    """NTT form of the constant polynomial m under the first l primes, from Python integers alone"""
    return np.array([[m % q] for q in primes[:l]], dtype=np.uint64) * np.ones((1, N), dtype=np.uint64)


def coeff_bound(values, N, scale):
    """2 sum|v| (slots / n_values) scale / N in the device's order of operations (nan / inf for a value that is not finite)"""
    v = [float(x) for x in np.atleast_1d(values)]
    total = 0.0
    for x in v:
        if not math.isfinite(x):
            return math.nan
        total += abs(x)
    return 2.0 * total * float((N // 2) // len(v)) * scale / float(N)


def device_accepts(values, N, scale):
    """the device encoder's rule, restated: every value finite and the coefficient bound below 2^62, the kernel's
    documented limit (no coefficient exceeds the bound: it is the triangle inequality over the N slot values)"""
    return coeff_bound(values, N, scale) < 2.0 ** 62
