"""evah_execute (eva_amd/csrc/scheduler.hip) on op lists CKKSCompiler never emits.  The contract of include/eva_hip.h —
"same ciphertexts as running the list op by op", and the ownership rule of the value table — on the lists of
tests/oplist.py: random ones (glue around every peephole pattern and near-miss, five flag policies, arbitrary residues),
the directed ones, lists with one invalid op, batched handles, captured graphs; and launch accounting that says the fused
forms are the ones that ran.  Every comparison is bit exact against oplist.walk (one oracle call per op, in list order).
The SEAL calls behind the ops: the reference's eva/seal/seal_executor.h:114-215.  EVA_OPLIST_SEEDS widens the random part."""
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest

import oplist as ol
from eva_amd import backend as be
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

SEEDS = int(os.environ.get("EVA_OPLIST_SEEDS", "64"))
OFF = {"EVAH_EW_FUSE": "0", "EVAH_WIN_FUSE": "0", "EVAH_FUSE_MUL": "0", "EVAH_FUSE_MUL2": "0", "EVAH_FUSE_MAC": "0"}
KNOBS = {
    "default": {},
    "off": OFF,
    "hoist0": {"EVAH_HOIST_MIN_TILES": "0"},
    "chain_step0": {"EVAH_CHAIN_STEP": "0"},
    "chain_batched0": {"EVAH_CHAIN_BATCHED": "0"},
    # one peephole off each, for the launch accounting
    "fuse_mul0": {"EVAH_FUSE_MUL": "0"},
    "fuse_mul20": {"EVAH_FUSE_MUL2": "0"},
    "ew_fuse0": {"EVAH_EW_FUSE": "0"},
    "hoist0_win_fuse0": {"EVAH_HOIST_MIN_TILES": "0", "EVAH_WIN_FUSE": "0"},
}
RANDOM_KNOBS = {"A": ["default", "off", "chain_step0", "chain_batched0"], "B": ["default", "off", "hoist0", "chain_step0", "chain_batched0"]}


class _G:
    """one context of a chain under one knob set, keys uploaded and warmed"""

    def __init__(self, chain, knobs):
        self.chain, self.knobs = chain, knobs
        self.N, self.primes = ol.CHAINS[chain][0], ol.primes_of(chain)
        self.g = be.Context(self.N, self.primes)
        self.keys = _keys(chain)
        self.g.upload_relin_key(self.keys["relin"])
        for st, key in self.keys["galois"].items():
            self.g.upload_galois_key(self.g.galois_elt_from_step(st), key)
        # first uses build the permutation tables (and the hoisted path's key copies): not part of any list's memory
        rng = np.random.default_rng(0)
        l = len(self.primes) - 1
        steps = ol.steps_of(chain)
        a = self.g.upload_ct(ol.rand_words(rng, self.primes, self.N, (2,), l), 2.0 ** ol.S)
        w = [self.g.upload_pt(ol.rand_words(rng, self.primes, self.N, (), l), 2.0 ** ol.S) for _ in steps]
        for st in steps:
            self.g.rotate(a, st).free()
        for h in self.g.rotate_many(a, steps) + self.g.rotate_weighted_sums([([(a, st) for st in steps], [w])]):
            h.free()
        self.g.relinearize_rescale(self.g.multiply(a, a), ol.DIV).free()
        for h in [a] + w:
            h.free()
        self.g.sync()


_ctxs = {}


@functools.lru_cache(maxsize=None)
def _keys(chain):
    return ol.make_keys(chain, np.random.default_rng(1000 + ord(chain)))


@functools.lru_cache(maxsize=None)
def _oracle(chain):
    return po.Oracle(ol.CHAINS[chain][0], ol.primes_of(chain))


def _ctx(chain, knobs, monkeypatch):
    """the knobs are read when a context is created: set first, then cached per (chain, knob set)"""
    if (chain, knobs) not in _ctxs:
        with monkeypatch.context() as m:
            for k, v in KNOBS[knobs].items():
                m.setenv(k, v)
            _ctxs[(chain, knobs)] = _G(chain, knobs)
    return _ctxs[(chain, knobs)]


@pytest.fixture(autouse=True)
def _stop_at_a_device_fault():
    """a HIP error is sticky: once a context reports one, nothing more of this module is started on the device"""
    yield
    for G in _ctxs.values():
        try:
            G.g.sync()
        except be.EvaHipError as e:
            pytest.exit(f"the device reported a fault ({e}): stopping", returncode=3)


def _hv(h):
    return h.h.value if isinstance(h.h, C.c_void_p) else h.h


def _baseline(g):
    """device bytes in use before a list's values go up (handles an earlier, failed test left to the collector first)"""
    gc.collect()
    g.sync()
    return g.mem_info()[0]


def _upload(g, values):
    out = {}
    for s, (kind, words, scale) in values.items():
        if kind == "pt":
            out[s] = g.upload_pt(words, scale)
        else:
            out[s] = g.upload_ct_batch(words, scale) if words.ndim == 4 else g.upload_ct(words, scale)
    return out


def _reference(lst, seed, edge=False):
    """(values, walk's values, live slots) — computed once per list, never written to"""
    values = ol.make_values(lst.chain, lst.placed, np.random.default_rng([77, seed]), edge=edge)
    ref, live = ol.walk(_oracle(lst.chain), lst.ops, values, _keys(lst.chain))
    for v in list(values.values()) + list(ref.values()):
        v[1].setflags(write=False)
    return values, ref, live


def _random(chain, seed, batch=1):
    lst = ol.random_oplist(seed, chain, batch)
    return (lst,) + _reference(lst, seed, edge=seed % 4 == 3)


@functools.lru_cache(maxsize=None)
def _directed(chain, name, batch=1):
    (lst,) = ol.directed(chain, batch, names=(name,))
    return (lst,) + _reference(lst, len(name))


def _check(G, lst, values, ref, live):
    """the property of the module docstring for one list on one context"""
    g = G.g
    base = _baseline(g)
    H = _upload(g, values)
    before = {s: _hv(h) for s, h in H.items()}
    got = g.execute(list(lst.ops), dict(H), n_vals=lst.n_vals)
    try:
        assert set(got) == live, (lst.name, "non-empty slots", sorted(set(got) ^ live))
        for s, h in got.items():
            kind, words, scale = ref[s]
            assert isinstance(h, be.Ciphertext if kind == "ct" else be.Plaintext), (lst.name, s)
            assert np.array_equal(h.download(), words), (lst.name, "slot", s, "differs from the walk")
            assert h.scale == scale, (lst.name, "scale of slot", s)
        # ownership: an unreleased caller value keeps its handle and its words, a released one is gone from the table, and
        # no two slots share a handle (Output slots hold their own)
        for s, h in H.items():
            if s in live:
                assert got[s] is h and _hv(h) == before[s], (lst.name, "caller slot", s, "changed hands")
                assert np.array_equal(h.download(), values[s][1]), (lst.name, "caller slot", s, "was written to")
            else:
                assert h.h is None
        assert len({_hv(h) for h in got.values()}) == len(got)
    finally:
        for h in got.values():
            h.free()
        for h in H.values():
            h.free()
    g.sync()
    assert g.mem_info()[0] == base, (lst.name, "device bytes still in use", g.mem_info()[0] - base)


# ---- (a) random lists ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(SEEDS))
@pytest.mark.parametrize("chain", ["A", "B"])
def test_random_lists(chain, seed, monkeypatch):
    """every knob set gives the walk's words, and therefore each other's"""
    lst, values, ref, live = _random(chain, seed)
    for knobs in RANDOM_KNOBS[chain]:
        try:
            _check(_ctx(chain, knobs, monkeypatch), lst, values, ref, live)
        except Exception as e:
            raise AssertionError(f"knobs {knobs}, policy {lst.policy}: {e}\n" + "\n".join(map(str, lst.ops))) from e


# ---- (b) directed lists ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ol.TEMPLATES))
@pytest.mark.parametrize("chain", ["A", "B"])
def test_directed_lists(chain, name, monkeypatch):
    lst, values, ref, live = _directed(chain, name)
    for knobs in ("default", "off") + (("hoist0",) if chain == "B" and lst.family == "win" else ()):
        try:
            _check(_ctx(chain, knobs, monkeypatch), lst, values, ref, live)
        except Exception as e:
            raise AssertionError(f"knobs {knobs}: {e}") from e


def test_output_outlives_the_value_another_reader_released(monkeypatch):
    """Output of a value that another op also reads and frees: free one handle, then download the other.  The other reader
    is a rotation by 0, whose result shares the released value's buffer with the Output, so three handles have stood on
    one buffer and each download below reads it after another of them has gone; then the same for two Outputs."""
    G = _ctx("A", "default", monkeypatch)
    for first in (0, 1):
        b = ol.Builder("A")
        x = b.add(b.x(0), b.x(1))
        pair = [b.out(x), b.rot(x, 0)]
        lst = ol._finish(b, "output+rot0", "", "compiler", None)
        assert x in ol.released(lst.ops)
        values, ref, live = _reference(lst, first)
        H = _upload(G.g, values)
        got = G.g.execute(list(lst.ops), dict(H), n_vals=lst.n_vals)
        assert set(got) == live and x not in got
        got[pair[first]].free()
        assert np.array_equal(got[pair[1 - first]].download(), ref[x][1])
        for h in list(got.values()) + list(H.values()):
            h.free()
    for name in ("own.output_and_freed_reader", "own.two_outputs"):
        lst, values, ref, live = _directed("A", name)
        H = _upload(G.g, values)
        got = G.g.execute(list(lst.ops), dict(H), n_vals=lst.n_vals)
        outs = [op[1] for op in lst.ops if op[0] == ol.OUTPUT]
        got[outs[0]].free()
        for s, h in got.items():
            if h.h is not None and s not in H:
                assert np.array_equal(h.download(), ref[s][1]), (name, s)
        for h in list(got.values()) + list(H.values()):
            h.free()


# ---- (c) one invalid op per list -------------------------------------------------------------------------------------
def _single(g, op, H):
    """op through the single entry point that stands for it (include/eva_hip.h: operand kinds select the call)"""
    code, _, s0, s1, imm = op[:5]
    a, b = H[s0], H.get(s1)
    if code in (ol.ADD, ol.SUB, ol.MUL):
        if code != ol.SUB and isinstance(a, be.Plaintext):
            a, b = b, a
        if isinstance(a, be.Plaintext):  # plain - cipher: the elementwise entry point is the one that takes such an op
            return g.elementwise_program([H[s0], H[s1]], [(code, 0, 1)], [2])[0]
        ct = isinstance(b, be.Ciphertext)
        if code == ol.ADD:
            return g.add(a, b) if ct else g.add_plain(a, b)
        if code == ol.SUB:
            return g.sub(a, b) if ct else g.sub_plain(a, b)
        return (g.square(a) if s0 == s1 else g.multiply(a, b)) if ct else g.multiply_plain(a, b)
    return {ol.NEG: lambda: g.negate(a), ol.ROTL: lambda: g.rotate(a, imm), ol.ROTR: lambda: g.rotate(a, -imm),
            ol.RELIN: lambda: g.relinearize(a), ol.RESCALE: lambda: g.rescale(a, imm), ol.MODSW: lambda: g.mod_switch(a)}[code]()


def _fails_like_the_single_call(G, lst, at, values):
    """g.execute(lst) raises what the single entry point raises for op `at` on the same operands; unflagged caller values
    are untouched; memory returns to its baseline once the caller frees what it still holds"""
    g = G.g
    op = lst.ops[at]
    ref, _ = ol.walk(_oracle(lst.chain), lst.ops[:at], values, _keys(lst.chain))
    base = _baseline(g)
    operands = _upload(g, {s: ref[s] for s in set(op[2:2 + ol.arity(op[0])])})
    with pytest.raises(be.EvaHipError) as single:
        _single(g, op, operands)
    want = str(single.value)
    del single
    for h in operands.values():
        h.free()
    H = _upload(g, values)
    with pytest.raises(be.EvaHipError) as whole:
        g.execute(list(lst.ops), dict(H), n_vals=lst.n_vals)
    have = str(whole.value)
    del whole
    gc.collect()  # (the handles the failed call had produced so far go with its frame)
    print(f"{lst.name}: single call: {want!r}; evah_execute: {have!r}")
    assert have == want, (lst.name, op)
    gone = ol.released(lst.ops)
    for s, h in H.items():
        if s not in gone:
            assert h.h is not None, (lst.name, "caller slot", s, "was taken")
            assert np.array_equal(h.download(), values[s][1]), (lst.name, "caller slot", s, "was written to")
    for h in H.values():
        h.free()
    g.sync()
    assert g.mem_info()[0] == base, (lst.name, "device bytes still in use", g.mem_info()[0] - base)


@pytest.mark.parametrize("seed", range(16))
@pytest.mark.parametrize("chain", ["A", "B"])
def test_one_invalid_op(chain, seed, monkeypatch):
    rng = np.random.default_rng([5, seed])
    fault = ol.FAULTS[seed % len(ol.FAULTS)]
    lst, at, _ = ol.inject_fault(ol.random_oplist(seed, chain), fault, rng)
    values = ol.make_values(chain, lst.placed, rng)
    for knobs in ("default", "off"):
        _fails_like_the_single_call(_ctx(chain, knobs, monkeypatch), lst, at, values)


def test_plain_minus_cipher(monkeypatch):
    """Sub(plaintext, ciphertext), the smallest list that failed before the scheduler named the case itself: evah_execute
    said "operand is not a ciphertext" where evah_elementwise_program and the reference say "Unsupported operation
    encountered" """
    b = ol.Builder("A")
    at = 2
    b.emit(ol.SUB, b.w(0), b.x(0), check=False)
    lst = ol._finish(b, "sub(pt, ct)", "", "compiler", None)
    assert lst.ops[at][0] == ol.SUB
    values = ol.make_values("A", lst.placed, np.random.default_rng(2))
    for knobs in ("default", "off"):
        _fails_like_the_single_call(_ctx("A", knobs, monkeypatch), lst, at, values)


def test_window_weight_of_another_limb_count(monkeypatch):
    """a tap whose weight has another limb count than the rotation's source: multiply_plain's error, not a window"""
    b = ol.Builder("A")
    r = [b.rot(b.x(0), 1), b.rot(b.x(0), 2)]
    p0 = b.mul(r[0], b.w(0))
    at = len(b.ops) + 1  # (the weight's marker op comes first)
    p1 = b.emit(ol.MUL, r[1], b.w(1, limbs=b.l - 1), check=False)
    b.emit(ol.ADD, p0, p1, check=False)
    lst = ol._finish(b, "win.weight_limbs", "", "compiler", None)
    assert lst.ops[at][0] == ol.MUL
    values = ol.make_values("A", lst.placed, np.random.default_rng(3))
    for knobs in ("default", "off"):
        _fails_like_the_single_call(_ctx("A", knobs, monkeypatch), lst, at, values)


def test_batched_and_single_operand_in_one_op(monkeypatch):
    b = ol.Builder("A", batch=3)
    x = b.neg(b.x(0))
    single = b._place(ol.T("ct", 2, b.l, ol.S, 1), ol.INPUT)
    at = len(b.ops)
    b.emit(ol.ADD, x, single, check=False)
    lst = ol._finish(b, "batched+single", "", "compiler", None)
    values = ol.make_values("A", lst.placed, np.random.default_rng(4))
    for knobs in ("default", "off"):
        _fails_like_the_single_call(_ctx("A", knobs, monkeypatch), lst, at, values)


# ---- (d) batched handles ---------------------------------------------------------------------------------------------
BATCHED = [n for n, t in ol.TEMPLATES.items() if t["family"] != "own"]  # every chain, window and expression list of (b)


@pytest.mark.parametrize("name", BATCHED)
def test_directed_lists_on_batched_handles(name, monkeypatch):
    """every ciphertext input a 3-instance handle (the plaintexts stay single): each instance equals the walk of that
    instance, the near-misses and the lists across the 64-entry chunk edge included"""
    lst, values, ref, live = _directed("A", name, batch=3)
    for knobs in ("default", "off", "chain_batched0"):
        try:
            _check(_ctx("A", knobs, monkeypatch), lst, values, ref, live)
        except Exception as e:
            raise AssertionError(f"knobs {knobs}: {e}") from e


@pytest.mark.parametrize("seed", range(16))
def test_random_lists_on_batched_handles(seed, monkeypatch):
    chain = "AB"[seed % 2]
    lst, values, ref, live = _random(chain, seed, batch=3)
    for knobs in ("default", "chain_batched0"):
        _check(_ctx(chain, knobs, monkeypatch), lst, values, ref, live)


# ---- (e) captured ----------------------------------------------------------------------------------------------------
def _captured(G, lst, values):
    g = G.g
    H = _upload(g, values)
    warm = g.execute(list(lst.ops), dict(H), n_vals=lst.n_vals)  # eager: fills the pool
    for s, h in warm.items():
        if s not in H:
            h.free()
    g.capture_begin()
    res = g.execute(list(lst.ops), dict(H), n_vals=lst.n_vals)
    graph = g.capture_end()
    try:
        for u in (1, 2):
            new = ol.make_values(lst.chain, lst.placed, np.random.default_rng([9, u]), edge=u == 2)
            for s, h in H.items():
                h.write(new[s][1])
            g.graph_launch(graph)
            ref, live = ol.walk(_oracle(lst.chain), lst.ops, new, _keys(lst.chain))
            assert set(res) == live
            for s, h in res.items():
                assert np.array_equal(h.download(), ref[s][1]), (lst.name, "replay", u, "slot", s)
    finally:
        g.graph_free(graph)
        for h in list(res.values()) + list(H.values()):
            h.free()


@pytest.mark.parametrize("seed", [s for s in range(10) if ol.POLICIES[s % len(ol.POLICIES)] != "inputs_too"])
def test_random_lists_captured_and_replayed(seed, monkeypatch):
    """(the lists that give their inputs away cannot be replayed: there is nothing left to write the next input into)"""
    lst, values, _, _ = _random("A", seed)
    _captured(_ctx("A", "default", monkeypatch), lst, values)


@pytest.mark.parametrize("name", ol.HEADLINE)
def test_headline_lists_captured_and_replayed(name, monkeypatch):
    lst, values, _, _ = _directed("A", name)
    _captured(_ctx("A", "default", monkeypatch), lst, values)


# ---- (f) the fused forms are the ones that ran -----------------------------------------------------------------------
def _launches(G, fn):
    """{kernel class: launches} of fn(g, handles): the profile counters of include/eva_hip.h around one (warm) call"""
    g = G.g
    g.profile(True)
    g.profile_reset()
    try:
        out = fn(g)
        g.sync()
        return {k: v[0] for k, v in g.profile_get().items()}, out
    finally:
        g.profile(False)


def _run(lst, values):
    def fn(g):
        res = g.execute(list(lst.ops), _upload(g, values), n_vals=lst.n_vals)
        for h in res.values():
            h.free()
    return fn


# the knob that turns one peephole off and nothing else, and the contexts to compare (windows: on chain B, where
# EVAH_HOIST_MIN_TILES=0 puts them on the hoisted + fused path).  Rescale -> Relinearize of a stored value is not here:
# evah_rescale_relinearize_many launches, class for class, what evah_rescale + evah_relinearize launch (3 inverse pass
# pairs, one digit pass, one inner product, 2 mod-down pass pairs — measured at N = 1024, l = 4), so these counters
# cannot tell the two apart; its near-misses are held by the slot and ownership checks above.
PEEPHOLE_OFF = {"mrr": ("A", "default", "fuse_mul0"), "mrr2": ("A", "default", "fuse_mul20"),
                "win": ("B", "hoist0", "hoist0_win_fuse0"), "expr": ("A", "default", "ew_fuse0")}
ACCOUNTED = [n for n, t in ol.TEMPLATES.items() if t["family"] in PEEPHOLE_OFF and t["fused"] is not None]


@pytest.mark.parametrize("name", ACCOUNTED)
def test_the_peephole_ran_or_did_not(name, monkeypatch):
    """A list the peephole applies to launches something else once the peephole's knob is off; a near-miss launches exactly
    the same kernels either way.  A near-miss that silently fuses and a pattern that silently stops fusing both fail
    here, even when the words agree."""
    chain, on, off = PEEPHOLE_OFF[ol.TEMPLATES[name]["family"]]
    lst, values, _, _ = _directed(chain, name)
    runs = []
    for knobs in (on, off):
        G = _ctx(chain, knobs, monkeypatch)
        _run(lst, values)(G.g)  # warm
        runs.append(_launches(G, _run(lst, values))[0])
    print(name, "fused" if lst.fused else "near-miss", runs)
    if lst.fused:
        assert runs[0] != runs[1], (name, "launches the same kernels with its peephole off", runs[0])
    else:
        assert runs[0] == runs[1], (name, "a near-miss takes part in the peephole", runs)


@pytest.mark.parametrize("n", [47, 48, 49, 100])
def test_a_dependent_chain_is_cut_at_the_depth_limit(n, monkeypatch):
    """n elementwise ops, each the only reader of the one before, then an Output: the scheduler keeps at most
    EXPR_MAX_DEPTH (48) unevaluated nodes in one dependent chain, so the list is ceil(n / 48) elementwise programs — one
    launch for 47 and 48, a second for the 49th op, three for 100 — and n launches with EVAH_EW_FUSE=0.  (The lists keep
    each 48-node program within the 48 polynomial pointers of one launch, see tests/oplist.py: a chain with a stored
    operand at every third node is cut by that limit first and runs as the separate calls, 47 launches for 47 ops.)"""
    lst, values, _, _ = _directed("A", f"expr.depth{n}")
    chain = [op for op in lst.ops if op[0] in ol.EW]
    readers = [sum(r[2 + k] == op[1] for r in lst.ops for k in range(ol.arity(r[0]))) for op in chain]
    assert len(chain) == n and readers == [1] * n and all(q[2] == p[1] for p, q in zip(chain, chain[1:]))
    counts = {}
    for knobs in ("default", "ew_fuse0"):
        G = _ctx("A", knobs, monkeypatch)
        _run(lst, values)(G.g)  # warm
        counts[knobs] = _launches(G, _run(lst, values))[0]
    print(lst.name, counts)
    assert counts["default"]["elementwise"] == -(-n // ol.EXPR_MAX_DEPTH), counts
    assert counts["ew_fuse0"]["elementwise"] == n, counts
    assert sum(counts["default"].values()) == counts["default"]["elementwise"]


def _same_launches_as(G, lst, values, call):
    """evah_execute(lst) launches, class for class, what call(g, handles of the caller-placed slots in slot order) does"""
    ins = sorted(lst.placed)

    def fn(g):
        H = _upload(g, values)
        for h in call(g, [H[s] for s in ins]):
            h.free()
    fn(G.g)
    _run(lst, values)(G.g)
    want, have = _launches(G, fn)[0], _launches(G, _run(lst, values))[0]
    print(lst.name, want, have)
    assert have == want, (lst.name, have, want)


def _chains_directly(lst):
    """the fused calls a list made of nothing but exclusive chains stands for: its products in list order, by the order of
    the chain and the limb count, at most 64 per call"""
    reader = {op[2]: op for op in lst.ops if op[0] in (ol.RELIN, ol.RESCALE)}
    slot = {s: i for i, s in enumerate(sorted(lst.placed))}

    def call(g, h):
        groups = {}
        for op in lst.ops:
            if op[0] == ol.MUL:
                groups.setdefault((reader[op[1]][0], lst.placed[op[2]].limbs), []).append((h[slot[op[2]]], h[slot[op[3]]]))
        outs = []
        for (second, _), pairs in groups.items():
            many = g.multiply_relinearize_rescale_many if second == ol.RELIN else g.multiply_rescale_relinearize_many
            for i in range(0, len(pairs), ol.KS_BATCH_MAX):
                chunk = pairs[i:i + ol.KS_BATCH_MAX]
                outs += many([p[0] for p in chunk], [p[1] for p in chunk], ol.DIV)
        return outs
    return call


CHAIN_LISTS = [f"{o}.{n}" for o in ("mrr", "mrr2") for n in ("exclusive", "shared_operand", "min_limbs", "x63", "x64", "x65")] + \
              ["both_orders_same_level"]


@pytest.mark.parametrize("name", CHAIN_LISTS)
def test_lists_of_chains_launch_what_the_fused_calls_launch(name, monkeypatch):
    """a list of exclusive chains = the fused entry point called directly on the same operands, launch for launch: one
    call per 64 chains of an order, a last call of one for the 65th"""
    lst, values, _, _ = _directed("A", name)
    _same_launches_as(_ctx("A", "default", monkeypatch), lst, values, _chains_directly(lst))


def test_other_fused_lists_launch_what_the_fused_calls_launch(monkeypatch):
    """the other peepholes against their entry points called directly (h: the caller-placed handles in slot order)"""
    def direct(name, chain, knobs, call):
        lst, values, _, _ = _directed(chain, name)
        _same_launches_as(_ctx(chain, knobs, monkeypatch), lst, values, call)
    # (evah_rescale_relinearize_many launches the classes evah_rescale + evah_relinearize launch, see PEEPHOLE_OFF: this
    # line holds the fused call to no more launches than that, it cannot tell whether the peephole applied)
    direct("resrel.input", "A", "default", lambda g, h: g.rescale_relinearize_many([h[0]], ol.DIV))
    direct("relres.one", "A", "default", lambda g, h: [g.relinearize_rescale(h[0], ol.DIV)])
    # windows, hoisted + fused: x0, then the weights in the order the sums use them
    window = lambda steps: (lambda g, h: g.rotate_weighted_sums([([(h[0], st) for st in steps], [[h[1], h[2], h[3]]])]))
    direct("win.weight_src1", "B", "hoist0", window([1, 2, 0]))
    direct("win.weight_src0", "B", "hoist0", window([1, 2, 0]))
    direct("win.rotate_right", "B", "hoist0", window([-1, -3, 2]))
    direct("win.two_sums_same_taps", "B", "hoist0",
           lambda g, h: g.rotate_weighted_sums([([(h[0], 1), (h[0], 4)], [[h[1], h[2]], [h[3], h[4]]])]))
    # x0 w0 w1 (w2) at the top level, x1 w0 w1 one level down: two calls, one per limb count
    direct("win.two_limb_counts", "B", "hoist0",
           lambda g, h: g.rotate_weighted_sums([([(h[0], 1), (h[0], 2)], [[h[1], h[2]]])]) +
           g.rotate_weighted_sums([([(h[4], 1), (h[4], 2)], [[h[5], h[6]]])]))
    # expressions: one evah_elementwise_program storing only what the Output reads
    M, N_, A = ol.MUL, ol.NEG, ol.ADD
    direct("expr.negate_size3", "A", "default", lambda g, h: g.elementwise_program(h, [(M, 0, 1), (N_, 2, 2)], [3]))
    direct("expr.add_size3_size2", "A", "default", lambda g, h: g.elementwise_program(h, [(M, 0, 1), (N_, 2, 2), (A, 3, 4)], [5]))
    direct("expr.plain_first", "A", "default", lambda g, h: g.elementwise_program(h, [(N_, 0, 0), (M, 2, 3), (A, 1, 4)], [5]))

    # Relinearize -> Rescale whose relinearized value an Add reads too: the three separate calls
    def separate(g, h):
        r = g.relinearize(h[0])
        return [r, g.rescale(r, ol.DIV), g.add(r, h[1])]
    direct("relres.also_add", "A", "default", separate)
