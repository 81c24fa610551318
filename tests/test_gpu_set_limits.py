"""Rotation sets and window sums at the limits of their launch tables ("limits of a launch set").

A rotation-set or window-sum call is cut by host planners into launch sets whose tables travel as kernel arguments:
evah_rotate_many's m_max = 64 / B rotations x B instances, hoist_tables' tiles (ten k_hoist_mac<TS, TR> shapes, HT_TILES
= 32 tiles per launch), the window chunk loop of evah_rotate_weighted_sums (WIN_MAX = 16 units, 64 pairs, one number of
sums and one linear form per chunk, the distinct * B <= 64 gate) and k_hoist_fix's HOIST_ZERO_CAP = 64 recorded zeros.
A wrong chunk offset, a stale table row or a < for <= gives wrong words for particular counts only, so every case here

  * compares EVERY instance of EVERY output word for word with the CPU oracle's rotate -> multiply_plain -> add, and
  * reads what ran from the EVAH_HOIST_DEBUG line of the call (rotation_sets.hip.h, hoist_debug_chunk) and asserts it.

The expected chunk and tile figures restate hoist_tables, evah_rotate_many's chunking and the window chunk loop on paper.
Context: N = 2048, chain [40, 20, 40, 41] (the smallest degree that hoists and that takes k_hoist_mac's MAP grid), Galois
keys of uniform random words for steps 1..64."""
import os

import numpy as np
import pytest

import test_gpu_parity as parity
from eva_amd import backend
from oracle import pyoracle as po
from test_gpu_hoist import CONFIGS, Env, _rand_pt, _uniform_pt, _window_oracle

pytestmark = pytest.mark.gpu

CFG = CONFIGS[0]
KNOBS = {"EVAH_HOIST": "1", "EVAH_HOIST_MIN_TILES": "0", "EVAH_WIN_FUSE": "1", "EVAH_FOLD_PA": "1", "EVAH_HOIST_DEBUG": "1",
         "EVAH_WIN_LINEAR": "1"}
ALL_STEPS = list(range(1, 65))
CT_SCALE, PT_SCALE = 2.0 ** 20, 2.0 ** 10

_keys = {}  # step -> key words, the same in every context of this module
_ctxs = {}


class LimitEnv(Env):
    """Env of test_gpu_hoist.py with this module's knobs pinned around the context's creation and all 64 keys uploaded"""

    def __init__(self, **extra):
        knobs = dict(KNOBS, **{k: str(v) for k, v in extra.items()})
        old = {k: os.environ.get(k) for k in knobs}
        os.environ.update(knobs)
        try:
            super().__init__(*CFG)
        finally:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        krng = np.random.default_rng(64)
        for st in ALL_STEPS:
            if st not in _keys:
                _keys[st] = np.stack([np.stack([np.stack([krng.integers(0, self.primes[i], size=self.N, dtype=np.uint64)
                                                          for i in range(self.k)]) for _ in range(2)])
                                      for _ in range(self.k - 1)])
            self.g.upload_galois_key(self.g.galois_elt_from_step(st), _keys[st])
        self.keys = _keys
        self.l = self.k - 1
        self._singles = []
        self._pool = None

    def rand(self, size, l):
        """uniform words, but c1 is the transform of coefficients drawn in [1, q): a uniformly random limb of the 20-bit
        prime has a stray zero digit coefficient in 0.2 % of draws (N / q), and the cases here assert the zero count"""
        a = super().rand(size, l)
        for i in range(l):
            a[1][i] = self.o.ntt(i, self.rng.integers(1, self.primes[i], size=self.N, dtype=np.uint64))
        return a

    def singles(self, n):
        """n single ciphertexts (words, handle), uploaded once per context"""
        while len(self._singles) < n:
            a = self.rand(2, self.l)
            self._singles.append((a, self.g.upload_ct(a, CT_SCALE)))
        return self._singles[:n]

    def batched(self, B):
        a = np.stack([self.rand(2, self.l) for _ in range(B)])
        return a, self.g.upload_ct_batch(a, CT_SCALE)

    def pool(self):
        """weights shared by the window cases: six general and six uniform plaintexts as (words, handle)"""
        if self._pool is None:
            gen = [_rand_pt(self, self.l) for _ in range(6)]
            uni = [_uniform_pt(self, self.l) for _ in range(6)]
            self._pool = {"general": [(w, self.g.upload_pt(w, PT_SCALE)) for w in gen],
                          "uniform": [(full, self.g.uniform_pt(v, PT_SCALE)) for full, v in uni]}
        return self._pool


def ctx(**extra):
    key = tuple(sorted(extra.items()))
    if key not in _ctxs:
        _ctxs[key] = LimitEnv(**extra)
    return _ctxs[key]


# ---- the debug line: "<kind>: k=v k=v ... | k=v ... | ..." -> (kind, head fields, [chunk fields])
def _calls(capfd):
    out = []
    for line in capfd.readouterr().err.splitlines():
        for kind in ("rotation set", "window sums"):
            if line.startswith(kind + ":"):
                parts = [dict(kv.split("=") for kv in p.split()) for p in line[len(kind) + 1:].split("|")]
                parts = [{k: (v if k == "tile" else int(v)) for k, v in d.items()} for d in parts]
                out.append((kind, parts[0], parts[1:]))
    return out


def _traced(capfd, fn):
    capfd.readouterr()
    res = fn()
    return res, _calls(capfd)


def _shape(chunks):
    return [(c["pairs"], c["tile"], c["tiles"]) for c in chunks]


def _check_rotations(e, inst, outs, steps):
    """inst [B][2][l][N]: every instance of every step against the oracle"""
    assert len(outs) == len(steps)
    for st, o in zip(steps, outs):
        got = o.download()
        if len(inst) == 1:
            got = got[None]
        assert got.shape[0] == len(inst)
        for b in range(len(inst)):
            assert np.array_equal(got[b], e.o.rotate(inst[b], st, e.keys[st])), f"step {st} instance {b}"


def _rotate_many(e, capfd, B, steps, inst=None):
    if inst is None:
        inst = np.stack([e.rand(2, e.l) for _ in range(B)])
    H = e.g.upload_ct(inst[0], CT_SCALE) if B == 1 else e.g.upload_ct_batch(inst, CT_SCALE)
    outs, calls = _traced(capfd, lambda: e.g.rotate_many(H, steps))
    _check_rotations(e, inst, outs, steps)
    assert len(calls) == 1 and calls[0][0] == "rotation set", calls
    return calls[0][1], calls[0][2]


def _rotate_pairs(e, capfd, plan, srcs):
    """plan: [(source index, step)], srcs: [(words, handle)]"""
    outs, calls = _traced(capfd, lambda: e.g.rotate_pairs([srcs[i][1] for i, _ in plan], [st for _, st in plan]))
    assert len(outs) == len(plan)
    for (i, st), o in zip(plan, outs):
        assert np.array_equal(o.download(), e.o.rotate(srcs[i][0], st, e.keys[st])), f"source {i} step {st}"
    assert len(calls) == 1 and calls[0][0] == "rotation set", calls
    return calls[0][1], calls[0][2]


# ---- A. every tile shape k_hoist_mac is dispatched with
# (shape, call, argument, tiles, tiles without padding): rotate_many of B instances by n steps, or rotate_pairs of the
# listed sources all by ONE step (a chunk with a single Galois element is what the TS x 1 column needs)
TILE_SHAPES = [
    ("1x2", "many", (1, 2), 1, 1),
    ("1x4", "many", (1, 3), 1, 0),  # three elements in a tile of four: one short tile
    ("2x2", "many", (2, 2), 1, 1),
    ("2x4", "many", (2, 3), 1, 0),
    ("3x2", "many", (3, 2), 1, 1),
    ("4x2", "many", (4, 2), 1, 1),
    ("1x1", "pairs", [0, 0], 2, 2),  # the same pair twice: two tiles of one pair, both outputs the oracle's
    ("2x1", "pairs", [0, 1, 0], 2, 1),
    ("3x1", "pairs", [0, 1, 2, 0], 2, 1),
    ("4x1", "pairs", [0, 1, 2, 3, 0], 2, 1),
]


@pytest.mark.parametrize("shape,call,arg,tiles,full", TILE_SHAPES, ids=[t[0] for t in TILE_SHAPES])
def test_every_tile_shape_is_reached(capfd, shape, call, arg, tiles, full):
    e = ctx()
    if call == "many":
        B, n = arg
        head, chunks = _rotate_many(e, capfd, B, [3, 5, 64][:n])
        pairs = B * n
    else:
        step = 5 if shape == "1x1" else 1
        head, chunks = _rotate_pairs(e, capfd, [(i, step) for i in arg], e.singles(4))
        pairs = len(arg)
    assert head["hoisted"] == 1 and head["zeros"] == 0, head
    assert len(chunks) == 1, chunks
    c = chunks[0]
    assert (c["pairs"], c["tile"], c["tiles"], c["full"], c["launches"]) == (pairs, shape, tiles, full, 1), c


# ---- B. rotate_many: m_max = 64 / B rotations x B instances per chunk
MANY_CHUNKS = [
    (1, 64, [(64, "1x4", 16)]),
    (3, 22, [(63, "3x2", 11), (3, "3x1", 1)]),
    (5, 13, [(60, "4x2", 12), (5, "4x1", 2)]),
    (21, 4, [(63, "4x2", 12), (21, "4x1", 6)]),
    (22, 3, [(44, "4x2", 6), (22, "4x1", 6)]),
    (32, 3, [(64, "4x2", 8), (32, "4x1", 8)]),
    (33, 2, [(33, "4x1", 9), (33, "4x1", 9)]),
    (64, 2, [(64, "4x1", 16), (64, "4x1", 16)]),
]


@pytest.mark.parametrize("B,n,want", MANY_CHUNKS, ids=[f"B{b}_n{n}" for b, n, _ in MANY_CHUNKS])
def test_rotate_many_chunks(capfd, B, n, want):
    e = ctx()
    # descending steps: the last chunk holds other keys than the first
    head, chunks = _rotate_many(e, capfd, B, ALL_STEPS[::-1][:n])
    assert head["hoisted"] == 1 and head["pairs"] == B * n and head["sources"] == B and head["zeros"] == 0, head
    assert _shape(chunks) == want, chunks
    assert all(c["launches"] == 1 for c in chunks), chunks


def test_rotate_many_refuses_65_steps_and_rotates_64_instances_unhoisted(capfd):
    e = ctx()
    a, H = e.batched(64)
    with pytest.raises(backend.EvaHipError, match=r"rotate_many handles 1\.\.64 rotations per call"):
        e.g.rotate_many(H, ALL_STEPS + [1])
    out, calls = _traced(capfd, lambda: e.g.rotate(H, 7))  # one step is never hoisted: 64 pairs through rot_chunk_plain
    _check_rotations(e, a, [out], [7])
    assert len(calls) == 1 and calls[0][1]["hoisted"] == 0 and [c["pairs"] for c in calls[0][2]] == [64], calls


# ---- C. rotate_pairs at 64 pairs
@pytest.mark.parametrize("hoist_map", [1, 0])
def test_rotate_pairs_ragged_64_takes_two_inner_product_launches(capfd, hoist_map):
    """63 sources with a step each and a 64th step on source 0: 63 tiles (none full) of shape 4x2, more than HT_TILES =
    32, so hoist_mac_launch refills the tile table from t0 = 32 for a second launch"""
    e = ctx(EVAH_HOIST_MAP=hoist_map)
    plan = [(i, i + 1) for i in range(63)] + [(0, 64)]
    head, chunks = _rotate_pairs(e, capfd, plan, e.singles(63))
    assert head["hoisted"] == 1 and head["sources"] == 63 and head["zeros"] == 0, head
    assert len(chunks) == 1, chunks
    c = chunks[0]
    assert (c["pairs"], c["sources"], c["elts"], c["tile"], c["tiles"], c["full"], c["launches"]) == (64, 63, 64, "4x2", 63, 0, 2), c


def test_rotate_pairs_rectangular_64_fills_its_tiles(capfd):
    e = ctx()
    plan = [(i, st) for i in range(4) for st in ALL_STEPS[10:26]]
    head, chunks = _rotate_pairs(e, capfd, plan, e.singles(4))
    assert head["hoisted"] == 1 and head["sources"] == 4, head
    assert _shape(chunks) == [(64, "4x2", 8)] and chunks[0]["full"] == 8 and chunks[0]["launches"] == 1, chunks


def test_rotate_pairs_64_distinct_sources_run_unhoisted_and_65_pairs_are_refused(capfd):
    e = ctx()
    srcs = e.singles(64)
    plan = [(i, 64 - i) for i in range(64)]  # 64 different keys
    head, chunks = _rotate_pairs(e, capfd, plan, srcs)
    assert head["hoisted"] == 0 and head["sources"] == 64 and [c["pairs"] for c in chunks] == [64], (head, chunks)
    with pytest.raises(backend.EvaHipError, match=r"rotate_pairs handles 1\.\.64 rotations per call"):
        e.g.rotate_pairs([srcs[0][1]] * 65, [1] * 65)


def test_rotate_pairs_with_mixed_strides_in_one_hoisted_set(capfd):
    """HoistMacTab::c1_ps per source: unstacked views of a mod-switched batched handle and a mod-switched single (poly
    stride of the level above), an unstacked view of a batched handle of this level and a standalone handle"""
    e = ctx()
    l = e.l
    up3, H3 = e.batched(2)
    low3 = [e.o.mod_switch(up3[b]) for b in range(2)]
    V3 = e.g.mod_switch(H3)
    b2 = np.stack([e.rand(2, l - 1) for _ in range(2)])
    H2 = e.g.upload_ct_batch(b2, CT_SCALE)
    up, single = e.rand(2, l), e.rand(2, l - 1)
    srcs = [(low3[0], V3.unstack(0)), (low3[1], V3.unstack(1)), (np.ascontiguousarray(b2[1]), H2.unstack(1)),
            (e.o.mod_switch(up), e.g.mod_switch(e.g.upload_ct(up, CT_SCALE))), (single, e.g.upload_ct(single, CT_SCALE))]
    plan = [(i, st) for st in (1, 33, 64) for i in range(5)]
    head, chunks = _rotate_pairs(e, capfd, plan, srcs)
    assert head["hoisted"] == 1 and head["l"] == l - 1 and head["sources"] == 5, head
    assert chunks[0]["pairs"] == 15 and chunks[0]["tile"] == "4x2", chunks


# ---- D. the window-sum chunk planner
def _run_windows(e, capfd, windows, B=1):
    """windows: [(terms, rows)], terms = [((words, handle), step)], rows = one list per sum of (words | None, handle |
    None) per term.  Every instance of every sum against the oracle; returns the outputs and the debug lines."""
    arg = [([(src[1], st) for src, st in terms], [[w[1] for w in row] for row in rows]) for terms, rows in windows]
    outs, calls = _traced(capfd, lambda: e.g.rotate_weighted_sums(arg))
    got = [o.download() for o in outs]
    assert len(got) == sum(len(rows) for _, rows in windows)
    i = 0
    for wi, (terms, rows) in enumerate(windows):
        for b in range(B):
            ref = _window_oracle(e, [(src[0][b] if B > 1 else src[0], st) for src, st in terms], [[w[0] for w in row] for row in rows])
            for f in range(len(rows)):
                assert np.array_equal(got[i + f][b] if B > 1 else got[i + f], ref[f]), f"window {wi} sum {f} instance {b}"
        i += len(rows)
    return outs, calls


def _fused_chunks(calls):
    assert len(calls) == 1 and calls[0][0] == "window sums" and calls[0][1]["fused"] == 1, calls
    return [(c["units"], c["pairs"]) for c in calls[0][2]]


def _rows(e, kind, n_terms, n_sums, shift=0):
    p = e.pool()[kind]
    return [[p[(j + 2 * s + shift) % len(p)] for j in range(n_terms)] for s in range(n_sums)]


WINDOW_PLANS = [
    # (id, windows as lists of steps (0 = the unrotated term), sums per window, weights, expected (units, pairs))
    ("17x2_uniform", [[w + 1, w + 2] for w in range(17)], 1, "uniform", [(16, 32), (1, 2)]),   # closed by WIN_MAX units
    ("17x2_general", [[w + 1, w + 2] for w in range(17)], 1, "general", [(16, 32), (1, 2)]),
    ("8x9", [list(range(w + 1, w + 10)) for w in range(8)], 2, "general", [(7, 63), (1, 9)]),  # closed by 64 pairs
    ("7x9_1_1", [list(range(w + 1, w + 10)) for w in range(7)] + [[20], [21]], 1, "uniform", [(8, 64), (1, 1)]),
    ("64_1", [ALL_STEPS, [5]], 1, "general", [(1, 64), (1, 1)]),
    ("63_and_unrotated", [ALL_STEPS[:31] + [0] + ALL_STEPS[31:63]], 2, "general", [(1, 63)]),
]


@pytest.mark.parametrize("name,plan,sums,kind,want", WINDOW_PLANS, ids=[p[0] for p in WINDOW_PLANS])
def test_window_chunks_close_at_units_and_pairs(capfd, name, plan, sums, kind, want):
    e = ctx()
    A = e.singles(1)[0]
    windows = [([(A, st) for st in steps], _rows(e, kind, len(steps), sums, shift=w)) for w, steps in enumerate(plan)]
    _, calls = _run_windows(e, capfd, windows)
    assert _fused_chunks(calls) == want, calls
    assert calls[0][1]["zeros"] == 0 and calls[0][1]["sources"] == 1
    assert all(c["F"] == sums and c["lin"] == (kind == "uniform") for c in calls[0][2]), calls


def test_window_of_65_terms_is_refused():
    e = ctx()
    A = e.singles(1)[0]
    with pytest.raises(backend.EvaHipError, match=r"a window has 1\.\.64 terms"):
        e.g.rotate_weighted_sums([([(A[1], st) for st in ALL_STEPS + [1]], [[None] * 65])])


def test_window_chunks_close_when_sums_or_linear_form_change(capfd):
    """(F=1, general), (F=2, general), (F=1, general), (F=1, uniform), (F=1, general): five chunks of one unit; the six
    sums come back in window order, each with its window's scale"""
    e = ctx()
    A = e.singles(1)[0]
    forms = [(1, "general"), (2, "general"), (1, "general"), (1, "uniform"), (1, "general")]
    windows, scales = [], []
    for w, (F, kind) in enumerate(forms):
        rows = []
        for _ in range(F):
            if kind == "general":
                words = [_rand_pt(e, e.l) for _ in range(2)]
                rows.append([(x, e.g.upload_pt(x, 2.0 ** (10 + w))) for x in words])
            else:
                rows.append([(full, e.g.uniform_pt(v, 2.0 ** (10 + w))) for full, v in (_uniform_pt(e, e.l) for _ in range(2))])
            scales.append(CT_SCALE * 2.0 ** (10 + w))
        windows.append(([(A, 2 * w + 1), (A, 2 * w + 2)], rows))
    outs, calls = _run_windows(e, capfd, windows)
    assert _fused_chunks(calls) == [(1, 2)] * 5, calls
    assert [(c["F"], c["lin"]) for c in calls[0][2]] == [(F, int(kind == "uniform")) for F, kind in forms], calls
    assert [o.info() for o in outs] == [(2, e.l, s) for s in scales]


def test_window_chunks_of_batched_handles_and_the_64_source_gate(capfd):
    e = ctx()
    # B = 24: one window of an unrotated and two rotated terms, two sums: 24 units of 2 pairs
    H = e.batched(24)
    _, calls = _run_windows(e, capfd, [([(H, 0), (H, 1), (H, 2)], _rows(e, "general", 3, 2))], B=24)
    assert _fused_chunks(calls) == [(16, 32), (8, 16)], calls
    assert calls[0][1]["sources"] == 24
    # B = 32 over two distinct sources: distinct * B = 64 is still fused
    H1, H2 = e.batched(32), e.batched(32)
    _, calls = _run_windows(e, capfd, [([(H1, 1), (H2, 2)], _rows(e, "general", 2, 1))], B=32)
    assert _fused_chunks(calls) == [(16, 32), (16, 32)], calls
    assert calls[0][1]["sources"] == 64 and [c["sources"] for c in calls[0][2]] == [32, 32], calls
    # B = 22 over three distinct sources: 66 > 64, the general form (one unhoisted rotate_many per source)
    Hs = [e.batched(22) for _ in range(3)]
    _, calls = _run_windows(e, capfd, [([(Hs[0], 1), (Hs[1], 2), (Hs[2], 3)], _rows(e, "general", 3, 1))], B=22)
    assert calls[0][0] == "window sums" and calls[0][1]["fused"] == 0 and calls[0][1]["sources"] == 3, calls
    assert [(k, h["hoisted"], h["pairs"]) for k, h, _ in calls[1:]] == [("rotation set", 0, 22)] * 3, calls


@pytest.mark.parametrize("B", [1, 2])
def test_general_form_chunks_more_than_64_rotated_terms(capfd, B):
    """three windows of 30 rotated terms with three sums each (more than two sums: never fused): 90 rotations go out as
    rotate_pairs calls of 64 + 26 pairs (B = 1) or rotate_many calls of 64 + 26 steps (B = 2)"""
    e = ctx()
    A = e.singles(1)[0] if B == 1 else e.batched(B)
    windows = [([(A, (30 * w + j) % 64 + 1) for j in range(30)], _rows(e, "general", 30, 3, shift=w)) for w in range(3)]
    _, calls = _run_windows(e, capfd, windows, B=B)
    assert calls[0][0] == "window sums" and calls[0][1]["fused"] == 0 and calls[0][1]["rotated"] == 90, calls
    assert [(k, h["hoisted"], h["pairs"]) for k, h, _ in calls[1:]] == [("rotation set", 1, 64 * B), ("rotation set", 1, 26 * B)], calls
    if B == 2:
        assert [[c["pairs"] for c in ch] for _, _, ch in calls[1:]] == [[64, 64], [52]], calls


# ---- E. zero digit coefficients at HOIST_ZERO_CAP and in later chunks
def _plant(e, a, counts, steps):
    """c1 of a [2][l][N] rebuilt from coefficient form drawn in [1, q) with exactly counts[limb] zeros per limb, at
    positions of which, for every step, at least one is sign-flipped by the rotation and one is not (index k goes to
    k * elt mod 2N, flipped iff bit logN is set): both arms of k_hoist_fix's test are taken"""
    logN = int(np.log2(e.N))
    elts = [po.galois_elt_from_step(e.N, st) for st in steps]
    total = sum(counts.values())
    for _ in range(1000):
        pos = {limb: e.rng.choice(e.N - 1, size=n, replace=False) + 1 for limb, n in counts.items()}
        allk = [int(k) for p in pos.values() for k in p]
        if total < 2 or all(len({(k * elt >> logN) & 1 for k in allk}) == 2 for elt in elts):
            break
    else:
        raise AssertionError("no positions with both a flipped and an unflipped zero for every step")
    for limb in range(a.shape[1]):
        x = e.rng.integers(1, e.primes[limb], size=e.N, dtype=np.uint64)
        x[pos.get(limb, [])] = 0
        assert np.count_nonzero(x == 0) == counts.get(limb, 0)
        a[1][limb] = e.o.ntt(limb, x)
    return total


def _split(total, parts):
    return [total // parts + (1 if i < total % parts else 0) for i in range(parts)]


@pytest.mark.parametrize("zeros,persist", [(63, None), (64, None), (65, 1), (65, 0)], ids=["63", "64", "65_persistent", "65_guarded"])
def test_zero_coefficients_at_the_correction_cap(capfd, zeros, persist):
    """k_hoist_fix corrects up to 64 recorded zeros, the fallback (both forms) recomputes from 65: no count is left to neither"""
    e = ctx() if persist is None else ctx(EVAH_FB_PERSIST=persist)
    steps = [1, 33, 64]
    a = e.rand(2, e.l)
    assert _plant(e, a, dict(enumerate(_split(zeros, e.l))), steps) == zeros
    head, chunks = _rotate_many(e, capfd, 1, steps, inst=a[None])
    assert head["hoisted"] == 1 and head["zeros"] == zeros, head
    assert _shape(chunks) == [(3, "1x4", 1)], chunks


@pytest.mark.parametrize("zeros", [64, 65])
def test_zero_coefficients_at_the_cap_spread_over_two_chunks(capfd, zeros):
    """B = 33 x 2 steps = two chunks; the zeros sit in instances 0, 17 and 32, the record is shared by both chunks"""
    e = ctx()
    steps = [2, 63]
    inst = np.stack([e.rand(2, e.l) for _ in range(33)])
    per = dict(zip((0, 17, 32), _split(zeros, 3)))
    for b in range(33):
        _plant(e, inst[b], dict(enumerate(_split(per.get(b, 0), e.l))), steps)
    head, chunks = _rotate_many(e, capfd, 33, steps, inst=inst)
    assert head["hoisted"] == 1 and head["zeros"] == zeros, head
    assert _shape(chunks) == [(33, "4x1", 9)] * 2, chunks


@pytest.mark.parametrize("zeros,sums,kind", [(3, 2, "general"), (70, 2, "general"), (70, 1, "uniform")],
                         ids=["3_corrected", "70_fallback", "70_fallback_linear"])
def test_zero_coefficients_in_the_second_chunk_of_a_window_call(capfd, zeros, sums, kind):
    """B = 24 x (an unrotated and two rotated terms) = chunks of 16 and 8 units; the zeros are in instance 20 only, which
    the second chunk serves: k_hoist_fix corrects chunk 1 through global source indices (3 zeros), both chunks take
    k_rot_fallback with their own window tables and ticket words (70 zeros)"""
    e = ctx()
    steps = [1, 64]
    inst = np.stack([e.rand(2, e.l) for _ in range(24)])
    for b in range(24):
        _plant(e, inst[b], dict(enumerate(_split(zeros if b == 20 else 0, e.l))), steps)
    H = (inst, e.g.upload_ct_batch(inst, CT_SCALE))
    _, calls = _run_windows(e, capfd, [([(H, steps[0]), (H, 0), (H, steps[1])], _rows(e, kind, 3, sums))], B=24)
    assert _fused_chunks(calls) == [(16, 32), (8, 16)], calls
    assert calls[0][1]["zeros"] == zeros, calls


# ---- F. evaluator calls at KS_BATCH_MAX = 64
def _each(out, n, ref_fn):
    d = out.download()
    assert d.shape[0] == n
    for b in range(n):
        assert np.array_equal(d[b], ref_fn(b)), f"instance {b}"


def test_evaluator_calls_on_a_batched_handle_of_64():
    e = parity.Env(*parity.CONFIGS[0])  # the smallest chain; own context: a relinearization key is installed
    l, n, s = e.k - 1, 64, 2.0 ** 10
    key = e.rand_key()
    e.g.upload_relin_key(key)
    a2, b2 = (np.stack([e.rand(2, l) for _ in range(n)]) for _ in range(2))
    a3 = np.stack([e.rand(3, l) for _ in range(n)])
    pt = e.rand(1, l)[0]
    A2, B2, A3 = (e.g.upload_ct_batch(x, s) for x in (a2, b2, a3))
    PT = e.g.upload_pt(pt, s)
    o = e.o
    _each(e.g.add(A2, B2), n, lambda b: o.add(a2[b], b2[b]))
    _each(e.g.multiply(A2, B2), n, lambda b: o.multiply(a2[b], b2[b]))
    _each(e.g.multiply_plain(A3, PT), n, lambda b: o.multiply_plain(a3[b], pt))
    _each(e.g.rescale(A2, 5), n, lambda b: o.rescale(a2[b]))
    _each(e.g.rescale(A3, 5), n, lambda b: o.rescale(a3[b]))
    _each(e.g.mod_switch(A3), n, lambda b: o.mod_switch(a3[b]))
    _each(e.g.relinearize(A3), n, lambda b: o.relinearize(a3[b], key))
    _each(e.g.relinearize_rescale(A3, 5), n, lambda b: o.rescale(o.relinearize(a3[b], key)))
    _each(e.g.rescale_relinearize(A3, 5), n, lambda b: o.relinearize(o.rescale(a3[b]), key))
    _each(e.g.multiply_relinearize_rescale(A2, B2, 5), n, lambda b: o.rescale(o.relinearize(o.multiply(a2[b], b2[b]), key)))
    _each(e.g.multiply_rescale_relinearize(A2, B2, 5), n, lambda b: o.relinearize(o.rescale(o.multiply(a2[b], b2[b])), key))


def test_many_calls_take_64_entries_and_refuse_65():
    e = parity.Env(*parity.CONFIGS[0])
    l, n, s = e.k - 1, 64, 2.0 ** 10
    key = e.rand_key()
    e.g.upload_relin_key(key)
    a2, b2 = ([e.rand(2, l) for _ in range(n)] for _ in range(2))
    a3 = [e.rand(3, l) for _ in range(n)]
    pts = [e.rand(1, l)[0] for _ in range(n)]
    A2, B2, A3 = ([e.g.upload_ct(x, s) for x in xs] for xs in (a2, b2, a3))
    PT = [e.g.upload_pt(x, s) for x in pts]
    o = e.o

    def same(outs, ref_fn):
        assert len(outs) == n
        for b, out in enumerate(outs):
            assert np.array_equal(out.download(), ref_fn(b)), f"entry {b}"

    def refused(fn, message):
        with pytest.raises(backend.EvaHipError, match=message):
            fn()

    more = lambda xs: xs + xs[:1]  # noqa: E731
    same(e.g.multiply_many(A2, B2), lambda b: o.multiply(a2[b], b2[b]))
    refused(lambda: e.g.multiply_many(more(A2), more(B2)), r"multiply_many handles 1\.\.64 products per call")
    same(e.g.multiply_plain_many(A3, PT), lambda b: o.multiply_plain(a3[b], pts[b]))
    refused(lambda: e.g.multiply_plain_many(more(A3), more(PT)), r"multiply_plain_many handles 1\.\.64 products per call")
    same(e.g.relinearize_many(A3), lambda b: o.relinearize(a3[b], key))
    refused(lambda: e.g.relinearize_many(more(A3)), r"relinearize_many handles 1\.\.64 ciphertexts per call")
    same(e.g.relinearize_rescale_many(A3, 5), lambda b: o.rescale(o.relinearize(a3[b], key)))
    refused(lambda: e.g.relinearize_rescale_many(more(A3), 5), r"relinearize_rescale_many handles 1\.\.64 ciphertexts per call")
    same(e.g.multiply_relinearize_rescale_many(A2, B2, 5), lambda b: o.rescale(o.relinearize(o.multiply(a2[b], b2[b]), key)))
    refused(lambda: e.g.multiply_relinearize_rescale_many(more(A2), more(B2), 5),
            r"multiply_relinearize_rescale_many handles 1\.\.64 products per call")
    # rescale_many counts polynomials: 128 per call
    same(e.g.rescale_many(A2, 5), lambda b: o.rescale(a2[b]))
    refused(lambda: e.g.rescale_many(more(A2), 5), "too many polynomials for one call")
    outs = e.g.rescale_many(A3[:42], 5)
    assert len(outs) == 42
    for b, out in enumerate(outs):
        assert np.array_equal(out.download(), o.rescale(a3[b])), f"entry {b}"
    refused(lambda: e.g.rescale_many(A3[:43], 5), "too many polynomials for one call")
