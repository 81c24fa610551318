"""Which launch form every caller of the key switch takes, pinned as launches per kernel class (profile_get) of one call
per caller, under the knob sets that test_gpu_knobs.py checks for words only.  Every form gives the same words, so words
cannot tell a form the library no longer takes from one it does; the launch counts can.

The literals of EXPECT were recorded by running measure() below on commit 8d0b947 ("Run the tail's two contiguous passes
inside the key-switch kernel"), the parent of the change that made ks_caps / ks_form (eva_amd/csrc) the one place that
chooses the form.  A launch count is not a measurement: the margin is equality.

Shape: N = 4096 with four 60-bit primes (l = 3), and one case at N = 1024 (a partial transform tile: neither the
small-launch form nor the mod-up kernel applies).  Every context has EVAH_HOIST=0, so rotate_many is the unhoisted rotation
set (rot_chunk_plain).  Every call's words are checked against the oracle as well.
  EVAH_FUSE_SMALL=48: with three products the digit transforms are 72 tiles (throughput size: the mod-up kernel) and the
  mod-down 36 (a small launch) — the special row's inverse pass rides a key switch that took the mod-up."""
import os

import numpy as np
import pytest

from eva_amd import backend
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

CLASSES = ("elementwise", "intt_pass1", "intt_pass2", "ksdigit_pass1", "ksdigit_pass2", "ks_mac", "moddown_pass1", "moddown_pass2",
           "ntt_pass1", "ntt_pass2")
CALLERS = ("relinearize", "relinearize_many3", "relinearize_rescale", "multiply_relinearize_rescale_many3", "multiply_rescale_relinearize",
           "rescale_relinearize", "rotate", "rotate_many")
STEPS = [1, 65, -3]
KNOB_SETS = {
    "defaults": (4096, {}),
    "FUSE_SPECIAL_INV=0": (4096, {"EVAH_FUSE_SPECIAL_INV": 0}),
    "KS_THREADS=256": (4096, {"EVAH_KS_THREADS": 256}),
    "KS_GROUPS=2": (4096, {"EVAH_KS_GROUPS": 2}),
    "MAC3=0": (4096, {"EVAH_MAC3": 0}),
    "FOLD_PA=0": (4096, {"EVAH_FOLD_PA": 0}),
    "FUSE_MAC=0": (4096, {"EVAH_FUSE_MAC": 0}),
    "FUSE_SMALL=0": (4096, {"EVAH_FUSE_SMALL": 0}),
    "FUSE_SMALL=0,KS_TAIL=1": (4096, {"EVAH_FUSE_SMALL": 0, "EVAH_KS_TAIL": 1}),
    "FUSE_SMALL=48": (4096, {"EVAH_FUSE_SMALL": 48}),
    "N1024": (1024, {}),
}
# EXPECT[knob set][caller] = launches per kernel class, in the order of CLASSES
EXPECT = {
    'defaults': {
        'relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rescale_relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
    },
    'FUSE_SPECIAL_INV=0': {
        'relinearize': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'rescale_relinearize': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate': (1, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 2, 0, 1, 0, 1, 1, 1, 0, 0),
    },
    'KS_THREADS=256': {
        'relinearize': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'rescale_relinearize': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate': (1, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 2, 0, 1, 0, 1, 1, 1, 0, 0),
    },
    'KS_GROUPS=2': {
        'relinearize': (0, 2, 1, 2, 0, 2, 1, 1, 0, 0),
        'relinearize_many3': (0, 2, 1, 2, 0, 2, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 3, 2, 0, 2, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 3, 3, 2, 0, 2, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 3, 1, 2, 0, 2, 2, 2, 0, 0),
        'rescale_relinearize': (0, 3, 1, 2, 0, 2, 2, 2, 0, 0),
        'rotate': (1, 2, 1, 2, 0, 2, 1, 1, 0, 0),
        'rotate_many': (1, 2, 1, 2, 0, 2, 1, 1, 0, 0),
    },
    'MAC3=0': {
        'relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rescale_relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
    },
    'FOLD_PA=0': {
        'relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 2, 0, 1, 0, 1, 2, 2, 0, 0),
        'rescale_relinearize': (0, 2, 0, 1, 0, 1, 2, 2, 0, 0),
        'rotate': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
    },
    'FUSE_MAC=0': {
        'relinearize': (0, 2, 1, 1, 1, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 2, 1, 1, 1, 3, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 3, 1, 1, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (1, 3, 3, 1, 1, 3, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 3, 1, 1, 1, 1, 2, 2, 0, 0),
        'rescale_relinearize': (0, 3, 1, 1, 1, 1, 2, 2, 0, 0),
        'rotate': (1, 2, 1, 1, 1, 1, 1, 1, 0, 0),
        'rotate_many': (1, 2, 1, 1, 1, 3, 1, 1, 0, 0),
    },
    'FUSE_SMALL=0': {
        'relinearize': (0, 2, 1, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 2, 1, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 2, 3, 1, 0, 1, 1, 1, 0, 0),
        'rescale_relinearize': (0, 2, 3, 1, 0, 1, 1, 1, 0, 0),
        'rotate': (1, 2, 1, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 2, 1, 1, 0, 1, 1, 1, 0, 0),
    },
    'FUSE_SMALL=0,KS_TAIL=1': {
        'relinearize': (0, 2, 1, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 2, 1, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 1, 0, 1, 0, 2, 1, 0, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 1, 0, 1, 0, 2, 1, 0, 0, 0),
        'multiply_rescale_relinearize': (0, 2, 3, 1, 0, 1, 1, 1, 0, 0),
        'rescale_relinearize': (0, 2, 3, 1, 0, 1, 1, 1, 0, 0),
        'rotate': (1, 2, 1, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 2, 1, 1, 0, 1, 1, 1, 0, 0),
    },
    'FUSE_SMALL=48': {
        'relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 2, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 2, 0, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rescale_relinearize': (0, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 1, 0, 1, 0, 1, 1, 1, 0, 0),
    },
    'N1024': {
        'relinearize': (0, 2, 2, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_many3': (0, 2, 2, 1, 0, 1, 1, 1, 0, 0),
        'relinearize_rescale': (0, 3, 3, 1, 0, 1, 1, 1, 0, 0),
        'multiply_relinearize_rescale_many3': (0, 3, 3, 1, 0, 1, 1, 1, 0, 0),
        'multiply_rescale_relinearize': (0, 3, 3, 1, 0, 1, 2, 2, 0, 0),
        'rescale_relinearize': (0, 3, 3, 1, 0, 1, 2, 2, 0, 0),
        'rotate': (1, 2, 2, 1, 0, 1, 1, 1, 0, 0),
        'rotate_many': (1, 2, 2, 1, 0, 1, 1, 1, 0, 0),
    },
}


def _ctx(N, primes, knobs):
    env = dict(knobs, EVAH_HOIST=0)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return backend.Context(N, primes)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class _Inputs:
    """keys, operands and the oracle's words of every call at one degree (the same for every knob set)"""

    def __init__(self, N):
        self.N = N
        self.primes = primes = po.coeff_modulus_create(N, [60] * 4)
        k = len(primes)
        l = self.l = k - 1
        self.div = 60
        o = po.Oracle(N, primes)
        rng = np.random.default_rng(N)

        def rand(prefix, nl):
            return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(nl)], axis=len(prefix))
        self.rk = rk = rand((l, 2), k)
        self.gks = {st: rand((l, 2), k) for st in STEPS}
        self.a, self.b = a, b = rand((2,), l), rand((2,), l)
        self.pairs = [(a, b), (b, b), (a, a)]
        self.m = [o.multiply(x, y) for x, y in self.pairs]
        chain = o.relinearize(o.rescale(self.m[0]), rk)
        self.want = {
            "relinearize": [o.relinearize(self.m[0], rk)],
            "relinearize_many3": [o.relinearize(m, rk) for m in self.m],
            "relinearize_rescale": [o.rescale(o.relinearize(self.m[0], rk))],
            "multiply_relinearize_rescale_many3": [o.op_triple(x, y, rk) for x, y in self.pairs],
            "multiply_rescale_relinearize": [chain],
            "rescale_relinearize": [chain],
            "rotate": [o.rotate(a, 65, self.gks[65])],
            "rotate_many": [o.rotate(a, st, self.gks[st]) for st in STEPS],
        }


_INPUTS = {}


def _inputs(N):
    if N not in _INPUTS:
        _INPUTS[N] = _Inputs(N)
    return _INPUTS[N]


def measure(name):
    """{caller: launches per kernel class} of one call per caller under a knob set; every call's words against the oracle"""
    N, knobs = KNOB_SETS[name]
    p = _inputs(N)
    g = _ctx(N, p.primes, knobs)
    try:
        g.upload_relin_key(p.rk)
        for st in STEPS:
            g.upload_galois_key(g.galois_elt_from_step(st), p.gks[st])
        up = [(g.upload_ct(x, 2.0 ** 30), g.upload_ct(y, 2.0 ** 30)) for x, y in p.pairs]
        M = [g.upload_ct(m, 2.0 ** 60) for m in p.m]
        A, B = up[0]
        calls = {
            "relinearize": lambda: [g.relinearize(M[0])],
            "relinearize_many3": lambda: g.relinearize_many(M),
            "relinearize_rescale": lambda: [g.relinearize_rescale(M[0], p.div)],
            "multiply_relinearize_rescale_many3": lambda: g.multiply_relinearize_rescale_many([u[0] for u in up], [u[1] for u in up], p.div),
            "multiply_rescale_relinearize": lambda: [g.multiply_rescale_relinearize(A, B, p.div)],
            "rescale_relinearize": lambda: [g.rescale_relinearize(M[0], p.div)],
            "rotate": lambda: [g.rotate(A, 65)],
            "rotate_many": lambda: g.rotate_many(A, STEPS),
        }
        counts = {}
        for caller in CALLERS:
            g.profile(True)
            g.profile_reset()
            outs = calls[caller]()
            g.sync()
            got = g.profile_get()
            g.profile(False)
            assert set(got) == set(CLASSES), got
            counts[caller] = tuple(got[c][0] for c in CLASSES)
            assert len(outs) == len(p.want[caller])
            for i, (x, want) in enumerate(zip(outs, p.want[caller])):
                assert np.array_equal(x.download(), want), f"{name}: {caller} result {i} differs from the oracle"
        return counts
    finally:
        g.close()


@pytest.mark.parametrize("name", list(KNOB_SETS))
def test_every_caller_takes_the_recorded_launch_form(name):
    got = measure(name)
    for caller in CALLERS:
        print(name, caller, dict(zip(CLASSES, got[caller])))
    assert got == EXPECT[name]
