"""tests/oplist.py without a GPU: its reference walk against the existing DAG walker, the generator's validity, the
coverage the random lists are built to have, and the released-set rule on lists whose answer is written out here."""
import collections

import numpy as np
import pytest

import oplist as ol
from eva import EvaProgram, Input, Output, Op
from oracle import pyoracle as po

SEEDS = 64  # the default of EVA_OPLIST_SEEDS (tests/test_gpu_oplist.py): the floors below are stated for it


def _lower(compiled, enc, o, k, N):
    """test_gpu_execute_abi._lower with the oracle's encoder for the Encode nodes: (ops, values, outputs)"""
    dump = compiled._dump()
    uses = collections.Counter(a for d in dump for a in d["operands"])
    raw, values, ops, seen = {}, {}, [], collections.Counter()
    for name, t in compiled.inputs.items():
        if name not in enc.names():
            continue
        kind, size, limbs, scale, data = enc.get(name)
        if kind in ("cipher", "plain"):
            values[t.index] = ("ct" if kind == "cipher" else "pt", data, scale)
        else:
            raw[t.index] = list(data) * (compiled.vec_size // len(data))
    for d in dump:
        t, op, a = d["id"], d["op"], d["operands"]
        if op == Op.Input:
            continue
        if op == Op.Constant:
            raw[t] = list(d["constant"]) * (compiled.vec_size // len(d["constant"]))
        elif op == Op.Encode:
            v = raw[a[0]]
            data = o.encode(k - 1 - d["encode_level"], np.array(v * (N // 2 // len(v)), dtype=np.float64), 2.0 ** d["encode_scale"])
            values[t] = ("pt", data, 2.0 ** d["encode_scale"])
        elif all(x in raw for x in a):
            x = [raw[i] for i in a]
            f = {Op.Add: lambda u, v: u + v, Op.Sub: lambda u, v: u - v, Op.Mul: lambda u, v: u * v}
            if op in f:
                raw[t] = [f[op](u, v) for u, v in zip(*x)]
            elif op == Op.Negate:
                raw[t] = [-u for u in x[0]]
            else:
                assert op in (Op.Rescale, Op.Relinearize, Op.ModSwitch, Op.Output), op
                raw[t] = list(x[0])
        else:
            flags = 0
            for s in a:
                seen[s] += 1
            for pos, s in enumerate(a[:2]):
                if seen[s] == uses[s] and s not in values and not (pos == 1 and a[0] == a[1]):
                    flags |= ol.FREE0 if pos == 0 else ol.FREE1
            imm = d.get("rotation", d.get("rescale_divisor", 0)) or 0
            ops.append((int(op), t, a[0], a[1] if len(a) > 1 else 0, int(imm), flags))
    return ops, values, {name: t.index for name, t in compiled.outputs.items()}


def _programs():
    from eva_amd.workloads import sobel
    poly = EvaProgram('p', vec_size=64)
    with poly:
        x = Input('x')
        Output('y', 3 * x ** 2 + 5 * x - 2)
    poly.set_output_ranges(20)
    poly.set_input_scales(30)
    sob = sobel(32, 32, 1024)
    sob.set_input_scales(25)
    sob.set_output_ranges(10)
    win = EvaProgram('three_windows_two_levels', vec_size=64)
    with win:
        x = Input('x')

        def conv(v, ws):
            acc = None
            for k, w in enumerate(ws):
                t = (v << k) * w
                acc = t if acc is None else acc + t
            return acc
        ix, iy = conv(x, [0.5, -1.0, 0.25]), conv(x, [0.125, 0.75, -0.5])
        Output('y', conv(ix * ix, [1.0, 1.0, 1.0]) + conv(ix * iy, [1.0, 0.5, 1.0]) - conv(iy * iy, [0.25, 1.0, 1.0]))
    win.set_output_ranges(20)
    win.set_input_scales(30)
    rng = np.random.default_rng(3)
    return {"polynomial": (poly, {'x': [i / 64.0 for i in range(64)]}),
            "sobel32": (sob, {'image': [((37 * i) % 256) / 255.0 for i in range(1024)]}),
            "three_windows_two_levels": (win, {'x': list(rng.uniform(-1, 1, 64))})}


@pytest.mark.parametrize("name", ["polynomial", "sobel32", "three_windows_two_levels"])
def test_walk_gives_the_dag_walkers_ciphertexts(name):
    """walk() on the lowered list = OracleExecutor.execute on the compiled program, bit for bit, scales included"""
    from eva.ckks import CKKSCompiler
    from eva.seal import generate_keys
    from oracle_executor import OracleExecutor
    prog, inputs = _programs()[name]
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    pub, sec = generate_keys(params, 3)
    enc = pub.encrypt(inputs, sig)
    N, primes = pub.poly_modulus_degree, list(pub.primes)
    o = po.Oracle(N, primes)
    ops, values, outs = _lower(compiled, enc, o, len(primes), N)
    galois = {}
    for op in ops:
        if op[0] in (ol.ROTL, ol.ROTR) and op[4]:
            st = op[4] if op[0] == ol.ROTL else -op[4]
            galois[st] = pub.galois_keys()[po.galois_elt_from_step(N, st)]
    got, live = ol.walk(o, ops, values, {"relin": pub.relin_key(), "galois": galois})
    ref = OracleExecutor(pub).execute(compiled, enc)
    checked = 0
    for oname, t in outs.items():
        if isinstance(ref[oname], list):
            continue
        assert np.array_equal(got[t][1], ref[oname].data), oname
        assert got[t][2] == ref[oname].scale
        checked += 1
    assert checked
    # compiler flags: every intermediate released, inputs and outputs left
    assert live == set(values) | {t for n, t in outs.items() if not isinstance(ref[n], list)}


def _lists(chain):
    return [ol.random_oplist(seed, chain) for seed in range(SEEDS)]


@pytest.mark.parametrize("chain", ["A", "B"])
def test_every_generated_list_is_valid_and_walks(chain):
    """every op of every list passes the type model (Builder.emit raises otherwise) and the oracle runs it; the walk
    defines every slot, with the model's size, limb count and scale; the op count stays within 10..40"""
    o = po.Oracle(ol.CHAINS[chain][0], ol.primes_of(chain))
    keys = ol.make_keys(chain, np.random.default_rng(1))
    tb, steps = ol.total_bits(chain), ol.steps_of(chain)
    for i, lst in enumerate(_lists(chain) + ol.directed(chain)):
        n_real = sum(1 for op in lst.ops if ol.arity(op[0]))
        if lst.name.startswith("random"):
            assert 10 <= n_real <= 40, (lst.name, n_real)
        rng = np.random.default_rng(5)
        values = ol.make_values(chain, lst.placed, rng, edge=i % 4 == 3)
        got, live = ol.walk(o, lst.ops, values, keys)
        types = dict(lst.placed)
        for op in lst.ops:
            if not ol.arity(op[0]):
                continue
            t = types[op[1]] = ol.infer(op, types, tb, steps)
            kind, words, scale = got[op[1]]
            assert kind == t.kind and scale == 2.0 ** t.ls, (lst.name, op)
            assert words.shape == ((t.size,) if kind == "ct" else ()) + (t.limbs, ol.CHAINS[chain][0]), (lst.name, op)
        assert set(got) == set(range(lst.n_vals)), lst.name
        assert live <= set(got)


def test_directed_lists_are_what_their_names_say():
    """the recogniser finds every directed list's own pattern in it (so the coverage count below counts the right thing)"""
    for chain in ("A", "B"):
        for lst in ol.directed(chain):
            assert lst.name in ol.patterns(lst.ops), (chain, lst.name)


@pytest.mark.parametrize("chain", ["A", "B"])
def test_coverage_floor(chain):
    """Over the default seeds every small pattern / near-miss occurs in >= 5 % of the lists and every flag policy in
    >= 10 %, by what the recogniser finds in the finished lists (not by what the generator meant to put there).  The wide
    lists (63..65 chains or terms, 47..100 dependent ops) cannot fit into 40 ops: they are directed lists only."""
    lists = _lists(chain)
    found = collections.Counter()
    for lst in lists:
        found.update(ol.patterns(lst.ops))
    meant = collections.Counter(lst.policy for lst in lists)
    print(f"\nchain {chain}: occurrences in {len(lists)} random lists")
    for name in ol.SMALL + ["policy." + p for p in ol.POLICIES]:
        print(f"  {name:36s} {found[name]:3d}  {100.0 * found[name] / len(lists):5.1f} %")
    for name in ol.SMALL:
        assert found[name] >= 0.05 * len(lists), (name, found[name])
    for p in ol.POLICIES:
        assert found["policy." + p] >= 0.10 * len(lists), (p, found["policy." + p])
        assert meant[p] >= 0.10 * len(lists), (p, meant[p])


def test_injected_faults_are_the_fault_they_name():
    """inject_fault puts exactly one invalid op into a list: everything before it is valid (checked inside), the op is
    refused by the check it names, and each fault kind can be injected into every default list"""
    for chain in ("A", "B"):
        for seed in range(16):
            rng = np.random.default_rng(seed)
            fault = ol.FAULTS[seed % len(ol.FAULTS)]
            bad, at, dst = ol.inject_fault(ol.random_oplist(seed, chain), fault, rng)
            assert bad.ops[at][1] == dst and len(bad.ops) > at


def test_released_set_rule():
    """A slot is released iff some reader names it with a FREE flag; whoever carries the flag, the release happens after
    the last reader.  Three lists, the answer written out."""
    I, NEG, ADD, OUT, F0, F1 = ol.INPUT, ol.NEG, ol.ADD, ol.OUTPUT, ol.FREE0, ol.FREE1
    # 0, 1 inputs; 2 = -0; 3 = 2 + 1 (frees 2); 4 = Output(3): nobody flags 3, nobody reads 4
    ops = [(I, 0, 0, 0, 4, 0), (I, 1, 0, 0, 4, 0), (NEG, 2, 0, 0, 0, 0), (ADD, 3, 2, 1, 0, F0), (OUT, 4, 3, 0, 0, 0)]
    assert ol.released(ops) == {2}
    assert ol.live_after(ops, {0: None, 1: None}) == {0, 1, 3, 4}
    # the flag on the FIRST of two readers of 2, and an input given away: 2 and 1 go, 0 stays
    ops = [(I, 0, 0, 0, 4, 0), (I, 1, 0, 0, 4, 0), (NEG, 2, 0, 0, 0, 0), (ADD, 3, 2, 1, 0, F0 | F1), (ADD, 4, 2, 0, 0, 0)]
    assert ol.released(ops) == {1, 2}
    assert ol.live_after(ops, {0: None, 1: None}) == {0, 3, 4}
    # no flags at all: everything stays, the dead value 3 included; Mul(a, a) flagged on SRC0 only releases a
    ops = [(I, 0, 0, 0, 4, 0), (NEG, 1, 0, 0, 0, 0), (NEG, 2, 1, 0, 0, 0), (NEG, 3, 1, 0, 0, 0)]
    assert ol.released(ops) == set() and ol.live_after(ops, {0: None}) == {0, 1, 2, 3}
    ops = [(I, 0, 0, 0, 4, 0), (NEG, 1, 0, 0, 0, 0), (ol.MUL, 2, 1, 1, 0, F0)]
    assert ol.released(ops) == {1} and ol.live_after(ops, {0: None}) == {0, 2}
