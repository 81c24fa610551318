"""Inputs that take the refresh's lift (client.hip k_refresh_lift, ckks_host.h refresh_lift_coeff) to its
arithmetic edges, shared by test_refresh_cpu.py and test_gpu_refresh.py, and a Python-integer account of which edges a
list of messages reaches.  No test of its own.

  edge_messages   N integers in (-Q_l / 2, Q_l / 2]
  coverage        which of the lift's branches a list takes, by name
  reachable       which of those names (chain, l, t) allows at all, with the reason for every one it does not

The lift reads everything off the mixed-radix digits v_i of U = M mod Q_l, U = sum_i v_i q_0..q_{i-1}.  The digits of
floor(Q_l / 2) = (Q_l - 1) / 2 are exactly (q_i - 1) / 2: sum_i (q_i - 1) q_0..q_{i-1} telescopes to Q_l - 1.  So a digit of
it plus or minus one is again a digit, and for every position there is a value on either side of the sign boundary whose
first differing digit, from the top, is that position."""
import numpy as np

from pyref import centered

# the chains of the GPU tests: name -> prime bits for coeff_modulus_create
CHAINS = {
    "mixed": [60, 30, 45, 50, 33, 60],
    "all60": [60] * 4,
    "w60x21": [60] * 21,
    "mixed21": [60, 30, 45, 50, 33] * 4 + [60],
    "b30x62": [30] * 62,                      # k = 62 is the longest chain a context takes: l = 61 the deepest level
}
T_ALL = (0, 1, 31, 62)
# (chain, l, the shifts t one test id runs) of the kernel-form test: each of <4>, <8>, <16> at its first and last level,
# <62> at its first and at the deepest level of a 21-prime chain, and at 32 and 61 digits.  l = 61 costs about 180
# transforms of the integer model per t, so its two shifts are two ids.
FORM_CASES = [(c, l, T_ALL) for c in ("w60x21", "mixed21") for l in (3, 4, 5, 8, 9, 16, 17, 20)]
FORM_CASES += [("b30x62", 32, (1, 31)), ("b30x62", 61, (0,)), ("b30x62", 61, (62,))]


def form_case_id(case):
    return f"{case[0]}-l{case[1]}-t" + "_".join(str(t) for t in case[2])


def form_levels_out(case):
    """the target levels L of a case: one prime, the value's own level, every prime but the last"""
    chain, l, ts = case
    return sorted({1, l, len(CHAINS[chain]) - 1})


def from_digits(digits, primes):
    U, pre = 0, 1
    for v, q in zip(digits, primes):
        assert 0 <= v < q
        U += v * pre
        pre *= q
    return U


def to_digits(U, primes):
    out = []
    for q in primes:
        out.append(U % q)
        U //= q
    assert U == 0
    return out


def position_values(primes, l):
    """for every digit position i < l, U just above floor(Q_l / 2) and U just below it among the values whose first
    differing digit from the top is digit i: (its digits above i, one more at i, zeros below), which is negative, and
    (its digits above i, one less at i, q_j - 1 below), which is not.  As centred integers, 2 l of them"""
    ps = primes[:l]
    Q = from_digits([q - 1 for q in ps], ps) + 1
    h = [(q - 1) // 2 for q in ps]
    assert from_digits(h, ps) == Q // 2
    out = []
    for i in range(l):
        up = from_digits([0] * i + [h[i] + 1] + h[i + 1:], ps)
        down = from_digits([q - 1 for q in ps[:i]] + [h[i] - 1] + h[i + 1:], ps)
        assert down <= Q // 2 < up
        out += [centered(up, Q), centered(down, Q)]
    return out


def edge_messages(primes, l, t, N, seed):
    """N integers in (-Q_l / 2, Q_l / 2]: the sign boundary, the ends, ties of the division and their neighbours in both
    signs, values whose mixed-radix digits exceed a smaller prime, the two values of every digit position that put the
    sign decision there, and random fill"""
    Q = 1
    for q in primes[:l]:
        Q *= q
    half = Q // 2
    lo = half + 1 - Q   # the most negative value, U = floor(Q / 2) + 1
    vals = [0, 1, -1, half, lo, half - 1, lo + 1]
    if t:
        tie, step = 1 << (t - 1), 1 << t
        for m in (0, 1, -1, -2, half // step - 1, -(half // step) + 1):
            for d in (-1, 0, 1):
                vals.append(tie + m * step + d)
    U, pre = 0, 1
    for q in primes[:l]:   # digits q_i - 1: v_0 ~ 2^60 is far above a 30-bit prime
        U += (q - 1) * pre
        pre *= q
        vals.append(centered(U, Q))
    at_positions = position_values(primes, l)
    assert all(lo <= v <= half for v in at_positions)   # the filter below drops none of them
    vals += at_positions
    vals = [v for v in vals if lo <= v <= half]
    assert len(vals) <= N, "the named values alone exceed N: none may be cut off"
    rng = np.random.default_rng(seed)
    width = max(64, 8 * l + 8)   # bytes: 64 bits more than Q_l has, so that the fill is uniform below Q_l at every level
    while len(vals) < N:
        vals.append(centered(int.from_bytes(rng.bytes(width), "little") % Q, Q))
    assert len(vals) == N
    return vals


def form_messages(primes, l, t, N=1024):
    """the list the kernel-form test refreshes at (l, t), and whose coverage the CPU test accounts for"""
    return edge_messages(primes, l, t, N, 7 * l + t)


def coverage(primes, l, t, M):
    """the names of the lift's branches the messages M take at level l and shift t, `primes` being the whole chain:

      sign_neg_at_<i>, sign_pos_at_<i>   the first digit from the top that differs from floor(Q_l / 2)'s is digit i, and it
                                         is larger (M < 0) / smaller (M >= 0)
      sign_undecided                     every digit equals: M = floor(Q_l / 2)
      m_neg, m_pos, m_zero               the sign of M itself
      d_neg, d_zero, d_pos, d_top        d = 2^(t-1) - rho, rho = (M + 2^(t-1)) mod 2^t, the exact division's correction:
                                         negative, zero, in (0, 2^(t-1)), and 2^(t-1) itself (rho = 0)
      d_over_prime_neg, d_over_prime_pos |d| is at least the chain's smallest prime, so that d mod q_j is a reduction
      digit_over_in_garner               a digit v_i is at least a later prime q_j, j < l: Garner reduces it first
      digit_over_in_lift                 a digit v_i is at least a prime q_j the value has no residue of, l <= j < k - 1"""
    ps = [int(q) for q in primes]
    k = len(ps)
    Q = from_digits([q - 1 for q in ps[:l]], ps[:l]) + 1
    h = [(q - 1) // 2 for q in ps[:l]]
    qmin = min(ps)
    later = [min(ps[i + 1:l]) for i in range(l - 1)]   # the smallest prime Garner reduces digit i under
    above = min(ps[l:k - 1], default=1 << 64)          # the smallest prime the lift reduces any digit under
    hit = set()
    for m in M:
        assert Q // 2 + 1 - Q <= m <= Q // 2
        v = to_digits(m % Q, ps[:l])
        for i in reversed(range(l)):
            if v[i] != h[i]:
                hit.add(f"sign_{'neg' if v[i] > h[i] else 'pos'}_at_{i}")
                assert (v[i] > h[i]) == (m < 0)
                break
        else:
            hit.add("sign_undecided")
        hit.add("m_neg" if m < 0 else "m_pos" if m > 0 else "m_zero")
        if t:
            hb = 1 << (t - 1)
            d = hb - (m + hb) % (1 << t)
            hit.add("d_neg" if d < 0 else "d_zero" if d == 0 else "d_top" if d == hb else "d_pos")
            if abs(d) >= qmin:
                hit.add("d_over_prime_neg" if d < 0 else "d_over_prime_pos")
        if any(x >= q for x, q in zip(v, later)):
            hit.add("digit_over_in_garner")
        if max(v) >= above:
            hit.add("digit_over_in_lift")
    return hit


def reachable(primes, l, t):
    """(the names coverage() can report for (chain, l, t) at all, {name it cannot: why}), for Q_l above 2^64: every
    remainder mod 2^t, t <= 62, then occurs on either side of zero"""
    ps = [int(q) for q in primes]
    k = len(ps)
    qmin = min(ps)
    assert from_digits([q - 1 for q in ps[:l]], ps[:l]) >= 1 << 64
    yes = {f"sign_{s}_at_{i}" for i in range(l) for s in ("neg", "pos")} | {"sign_undecided", "m_neg", "m_pos", "m_zero"}
    no = {}
    for name in ("d_neg", "d_zero", "d_pos", "d_top", "d_over_prime_neg", "d_over_prime_pos"):
        if t == 0:
            no[name] = "t = 0 divides by nothing: no remainder is formed"
        elif t == 1 and name in ("d_neg", "d_pos"):
            no[name] = "t = 1: rho is 0 or 1, d is 1 or 0"
        elif name == "d_over_prime_pos" and (1 << (t - 1)) < qmin:
            no[name] = "d <= 2^(t-1) is below the smallest prime"
        elif name == "d_over_prime_neg" and (1 << (t - 1)) - 1 < qmin:
            no[name] = "-d <= 2^(t-1) - 1 is below the smallest prime"
        else:
            yes.add(name)
    # the largest digit at position i is q_i - 1: it reaches q_j exactly when q_i > q_j
    if any(ps[i] > ps[j] for j in range(l) for i in range(j)):
        yes.add("digit_over_in_garner")
    else:
        no["digit_over_in_garner"] = "no prime below level l is smaller than one before it"
    if any(ps[i] > ps[j] for j in range(l, k - 1) for i in range(l)):
        yes.add("digit_over_in_lift")
    else:
        no["digit_over_in_lift"] = "no prime from l to k - 2 is smaller than one below l"
    return yes, no
