"""The looped contiguous pass (ntt_loop_kernel) at every pass size, under every op that reaches it, in every walk shape.

At throughput size every contiguous transform pass is ntt_loop_kernel: a 64-thread workgroup stages the local twiddle
heaps of its 256-coefficient tile in LDS once and walks up to `nloop` jobs along the op's loop axis.  launch_loop_pass
(launch.hip.h) keeps small launches out of it, and the kernel reports the profile class of ntt_pass_kernel, so the other
modules neither reach it nor could tell.  Here
  * EVAH_LOOP_MIN_WGS=0 EVAH_LOOP_TARGET_WGS=0 (FORCE) make every contiguous launch of at least EVAH_LOOP_MIN jobs loop with
    nloop = min(EVAH_LOOP_N, count), whatever the degree;
  * Context.loop_stats() says what looped: launches per class (inverse pass 1, plain forward pass 2, key-switch digit pass
    2, mod-down pass 2), the jobs along the loop axes and the walks along them;
  * loop_plan() restates the launch rule and _Model the contiguous launches of every evaluator call, read off the launch
    sites (table below).  _Counted wraps a context: the counter difference over EVERY call must be what loop_plan gives for
    that call's launches, and when the context is closed the sites the id is there for must be among those that looped.
    An id whose kernel did not run fails, as an id of the other modules does on its launch counts.
    The counters hold classes, jobs and walks, not ops: two launches of one class and grid (OpPlain and OpMulIntt, both
    (1, l, n)) look alike to them, so a site's NAME below is the model's word for the launch the library made there.
Every word is compared bit for bit with oracle.pyoracle (_same).
Keys: q - 1 in every word, as the issue of this module asks, AND q - 1 mixed with zeros (a second pass per id on fewer
words; the walks use mixed keys only).  With every key word at q - 1 = -1 the key-switch result is -(t_0 + ... + t_{l-1}) / P:
coefficients between -l and 0 WHATEVER the digits t_J are, as long as the NTT-form target and the digits belong to one
polynomial, and the rescale of relinearize_rescale and of the fused products rounds that away.  Such keys show a wrapped
word, which is what they are for, but not a wrong digit set: a build that swapped the two raw operands of a pair in
OpMulIntt::finish_load (the later jobs of a walk then transform d2(-X) and store it as d2) gave the oracle's words in every
form that stores d2.  Mixed keys do not commute with that, and the default-form ids fail on such a build.

Contiguous launches per call (n = instances or entries of the launch set, l = limbs, k = primes; grid as Op::grid gives
it, x/y/z, before the tile factor; `axis` is Op::loop_axis, the extent along it is `count`).  Forms: see FORMS.
  call                         form                   op              dir  axis  grid
  every key switch             any                    OpPlain         inv  2     (1, l, n)      digits; pass1_only in small / modup
  (relinearize, rotate, ...)   EVAH_FUSE_MAC=0        OpKsDigit       fwd  0     (l, l + 1, n)  switch_key_products: ntt_forward<OpKsDigit>
    then its mod-down          not special_inv        OpPlain         inv  2     (1, 1, 2 n)    special rows (inverse_then_forward)
                               any                    OpModDown       fwd  2     (1, l, 2 n)
  relinearize_rescale(_many)   as above, then the tail:
    TAIL_THREE                 modup                  OpTailIntt      inv  2     (1, 2, 2 n)
                                                      OpRRFolded      fwd  2     (1, l - 1, 2 n)
    six launches               small, sliced, tail6   OpPlain         inv  2     (1, 1, 2 n)    special rows
      folded (default)                                OpRRLastFolded  inv  1     (1, 2 n, 1)
                                                      OpRRFolded      fwd  2     (1, l - 1, 2 n)
      EVAH_FUSE_MAC=0 / FOLD_PA=0                     OpRRLast(Mul)   inv  1     (1, 2 n, 1)
                                                      OpRR(Mul)       fwd  2     (1, l - 1, 2 n)
    TAIL_KS_SLICES             (ks_tail)              none: both contiguous passes are inside ks_inner_kernel
  multiply_relinearize_rescale(_many): the same with OpMulIntt (1, l, n) for OpPlain's digits (d2 stored unless
    EVAH_FOLD_PA=0); a batched handle, or EVAH_FUSE_MAC=0: multiply + relinearize_rescale
  multiply_rescale_relinearize(_many), rescale_relinearize(_many), n = handles x instances:
    chain step                 N >= 2048, folded      OpChainIntt     inv  2     (1, l + 2, n)   chain_step, step 1
                               not special_inv        OpPlain         inv  2     (1, 1, 2 n)     chain_step: special rows, md_small / not
                                                      OpModDown       fwd  2     (1, l - 1, 2 n) chain_step: last launch
    otherwise (products)                              OpMulPolyIntt   inv  1     (1, 3 n, 1)
                                                      OpModDownMul    fwd  2     (1, l - 1, 3 n) then relinearize at l - 1
    otherwise (stored)         rescale + relinearize per handle
  rescale, rescale_many        any                    OpPlain         inv  2     (1, 1, polys)
                                                      OpModDown       fwd  2     (1, l - 1, polys)
  rotate_many, >= 2 steps, N >= 2048 (hoisted; EVAH_HOIST_MIN_TILES=0 here), B instances, chunks of np pairs:
    first use of an element                           OpPlain         fwd  2     (1, k, 1)       hoist_sign
    once per set                                      OpPlainZ        inv  2     (1, l, B)       records zero coefficients
                                                      OpKsDigit       fwd  0     (l, l + 1, B)
    per chunk                                         OpPlainG        inv  2     (1, 1, 2 np)    rot_mod_down
                                                      OpModDownG      fwd  2     (1, l, 2 np)
  rotate_weighted_sums, fused window (N >= 2048, EVAH_FOLD_PA=1): the hoisted set's first three lines, then per chunk
                               any                    OpPlainG        inv  2     (1, 1, 2 np)    the window's special rows, small / not
    (its forward passes are the window kernels' own); general form: rotate_pairs / rotate_many, then elementwise sums
inverse_then_forward launches the same two contiguous passes in both of its branches (only the strided ones fuse), so the
forms differ in WHICH sites run, not in the grids; `special_inv` (the special rows' inverse pass inside ks_inner_kernel)
holds for small mod-downs of fused key switches unless EVAH_FUSE_SPECIAL_INV=0.

Sites and the ids that loop them (test_sites_loop_on_worst_case_words[N-chain-form], N = 1024, 4096, 16384, 65536 for
P = 5, 6, 7, 8; MUST below is checked per id):
  ntt_inverse<OpPlain> / <OpMulIntt> pass1_only, d2 stored     default (N >= 2048)
  the same, both passes (not pass1_only)                         two_launch; every form at N = 1024
  OpMulIntt without d2, OpRRLastMul / OpRRMul                    fold_pa0
  ntt_forward<OpKsDigit>, OpRRLast / OpRR                        unfused (and every hoisted set, N >= 2048)
  OpTailIntt, OpRRFolded after ntt_tail_kernel                   nosmall (N >= 2048)
  OpRRLastFolded / OpRRFolded, six launches                      default, two_launch, tail6
  chain_step's OpChainIntt and OpModDown                         default, nosmall, special_inv0 (N >= 2048)
  chain_step's special rows (OpPlain), md_small                  special_inv0 (N >= 2048);  not md_small: nosmall
  the fused window's OpPlainG, small launch                      default;  not small: nosmall (N >= 2048)
  OpPlainZ, OpPlainG / OpModDownG of a rotation set              every form but fold_pa0's window (N >= 2048)
  OpMulPolyIntt / OpModDownMul                                   chain0, unfused, fold_pa0; every form at N = 1024
  rescale's and the mod-down's inverse_then_forward, both branches   default | nosmall
Not reachable at N = 1024 (P = 5) in any form: OpTailIntt (the mod-up and tail kernels need 2048-coefficient tiles), OpChainIntt
and the rest of chain_step (chain_step_applies asks N >= 2048), OpPlainZ / OpPlainG / OpModDownG and the fused window
(hoist_wanted asks N >= 2048); pass1_only never holds there (no small-launch form on partial tiles).  N = 2048 has the same
contiguous pass size (P_b = 5) and all of these: the forms default, nosmall and special_inv0 run there as well.
OpPlainZ's launch has one job per source: it loops for batched handles, and for a single ciphertext under EVAH_LOOP_MIN=1
(test_zero_coefficient_record_under_the_looped_inverse_pass: N = 2048, 4096, 16384, 65536).  rescale's own
inverse_then_forward is not among _check_key_switches' calls: test_rounding_ties_loop runs it, in both branches.

Walk shapes (N = 4096, [60] * 4; test_walks_*): batches of B = 1, 2, 3 instances that all hold different words under
EVAH_LOOP_N = 2, 3, 4, 5, 8 (6 = 4 + 2, 6 = 5 + 1: ragged last walks of two jobs and of one; 8: one walk of everything);
OpKsDigit's skipped jobs with l = 5 under EVAH_LOOP_N = 2, 3, 8; EVAH_LOOP_MIN=1 (one job, no prefetch: the knob is not
clamped, the words are the same); the halving rule at the default EVAH_LOOP_TARGET_WGS on count = 6 (EVAH_LOOP_N = 7: nloop
min(7, 6) = 6 -> 3 -> 2; 5 -> 3 -> 2).
The default gate (no knobs) is checked at N = 65536 on both sides of EVAH_LOOP_MIN_WGS = 2048, and at the metric shape.
Two things about what can be seen where.  At P = 8 a 256-coefficient tile is ONE sub-transform (logC = 0), so the sub-transform
term `sb` of the twiddle staging index is always 0 there: an index without it is wrong at P = 5, 6, 7 only, and the 2^16 ids
cannot tell.  And the default gate is not shut for every small shape: at N = 4096 a hoisted set's OpKsDigit launch
(l, l + 1, 1) has 16 (l + 1) ceil(l / 2) workgroups, 2048 from l = 15 on, so test_gpu_extremes.py's l >= 15 ids already run
that one launch in the looped kernel at P = 6."""
import hashlib

import numpy as np
import pytest

import test_gpu_extremes as tge
from oracle import pyoracle as po
from test_gpu_extremes import _check_key_switches, _check_rounding_ties, _ctx, _forms, _keys, _same, _ties
from test_gpu_extremes_degrees import _ORACLE, _oracle, _searched_form

pytestmark = pytest.mark.gpu

INV, NTT, KSD, MD = 0, 1, 2, 3  # Context.loop_stats()[0..3]
FORCE = {"EVAH_LOOP_MIN_WGS": 0, "EVAH_LOOP_TARGET_WGS": 0}
KS_BATCH_MAX, WIN_MAX = 64, 16


def loop_plan(ext, axis, N, knobs):
    """launch_loop_pass's decision for a launch of grid `ext` (before the tile factor) whose jobs of one prime lie along
    `axis`: None (ntt_pass_kernel) or (count, nloop)"""
    loop_n, loop_min = int(knobs.get("EVAH_LOOP_N", 8)), int(knobs.get("EVAH_LOOP_MIN", 2))
    min_wgs, target = int(knobs.get("EVAH_LOOP_MIN_WGS", 2048)), int(knobs.get("EVAH_LOOP_TARGET_WGS", 8192))
    count = ext[axis]
    if not loop_n or count < loop_min or N < 256:
        return None
    others = ext[0] * ext[1] * ext[2] // count * (N // 256)
    if others * ((count + 1) // 2) < min_wgs:
        return None
    nloop = min(loop_n, count)
    while nloop > 2 and others * ((count + nloop - 1) // nloop) < target:
        nloop = (nloop + 1) // 2
    return count, nloop


def plan_stats(launches, N, knobs):
    """what loop_stats() must grow by over `launches` = [(site, class, grid, axis)], and the sites that loop"""
    out, sites = [0] * 6, set()
    for site, cls, ext, axis in launches:
        p = loop_plan(ext, axis, N, knobs)
        if p is not None:
            count, nloop = p
            out[cls] += 1
            out[4] += count
            out[5] += (count + nloop - 1) // nloop
            sites.add(site)
    return tuple(out), sites


class _Model:
    """The contiguous transform launches of each evaluator call of a context (the module docstring's table), from its
    knobs and what it reports of itself.  Hoisted sets build a table with a transform at the first use of an element."""

    def __init__(self, g, knobs):
        self.g, self.N, self.k, self.knobs = g, g.N, g.k, knobs
        t = lambda name, default: int(knobs.get(name, default))  # noqa: E731
        self.fuse_mac, self.fold_pa = t("EVAH_FUSE_MAC", 1) != 0, t("EVAH_FOLD_PA", 1) != 0
        self.fuse_small, self.modup = t("EVAH_FUSE_SMALL", 2048), t("EVAH_MODUP", 1) != 0
        self.tail_fuse, self.chain = t("EVAH_TAIL_FUSE", 1) != 0, t("EVAH_CHAIN_STEP", 1) != 0
        self.fuse_special, self.win_fuse = t("EVAH_FUSE_SPECIAL_INV", 1) != 0, t("EVAH_WIN_FUSE", 1) != 0
        self.hoist, self.hoist_min = t("EVAH_HOIST", 1) != 0, t("EVAH_HOIST_MIN_TILES", 2048)
        self.fold = self.fold_pa and self.fuse_mac
        self.ks_tail_on, self.ks_tail_min = g.ks_tail()
        self.signs = set()

    # ---- launch.hip.h
    def small(self, fwd_jobs):  # fuse_small_launch
        return bool(self.fuse_small) and self.N >= 2048 and fwd_jobs * (self.N // 2048) <= self.fuse_small

    def digits(self, l, n):  # ks_form
        if not self.fuse_mac:
            return "unfused"
        if self.small(n * (l + 1) * l):
            return "small"
        return "modup" if self.modup and self.N >= 2048 else "sliced"

    def special_inv(self, l, n):
        return self.small(2 * n * l) and self.fuse_special and self.fuse_mac

    def products(self, l, n, mul=False):  # switch_key_products
        d = self.digits(l, n)
        how = "pass1" if d in ("small", "modup") else "both passes"
        op = ("OpMulIntt+d2" if self.fold else "OpMulIntt") if mul else "OpPlain digits"
        out = [(f"{op} inv ({how})", INV, (1, l, n), 2)]
        if d == "unfused":
            out.append(("OpKsDigit fwd", KSD, (l, l + 1, n), 0))
        return out

    def mod_down(self, l, n, special_inv, what="mod-down", op="OpModDown"):  # inverse_then_forward<OpPlain, MD>
        branch = "small" if self.small(2 * n * l) else "full"
        out = [] if special_inv else [(f"OpPlain special inv ({what}, {branch})", INV, (1, 1, 2 * n), 2)]
        return out + [(f"{op} fwd ({what}, {branch})", MD, (1, l, 2 * n), 2)]

    def key_switch(self, l, n):  # switch_key_mod_down
        return self.products(l, n) + self.mod_down(l, n, self.special_inv(l, n))

    def chunks(self, batch):
        return [min(KS_BATCH_MAX, batch - b0) for b0 in range(0, batch, KS_BATCH_MAX)]

    # ---- keyswitch.hip
    def relin_rescale_core(self, l, n, mul):
        d = self.digits(l, n)
        out = self.products(l, n, mul)
        if self.ks_tail_on and l >= 2 and d == "modup" and 2 * n * (self.N // 256) >= self.ks_tail_min:
            return out  # TAIL_KS_SLICES
        if self.fold and self.tail_fuse and d == "modup":
            return out + [("OpTailIntt inv", INV, (1, 2, 2 * n), 2), ("OpRRFolded fwd (three)", MD, (1, l - 1, 2 * n), 2)]
        mode = "Folded" if self.fold else ("Mul" if mul else "")
        return out + [("OpPlain special inv (tail)", INV, (1, 1, 2 * n), 2), (f"OpRRLast{mode} inv", INV, (1, 2 * n, 1), 1),
                      (f"OpRR{mode} fwd", MD, (1, l - 1, 2 * n), 2)]

    def chain_applies(self):
        return self.chain and self.fold and self.N >= 2048

    def chain_step(self, l, n):
        lp = l - 1
        out = [("OpChainIntt inv", INV, (1, l + 2, n), 2)]
        if not self.special_inv(lp, n):
            out.append((f"OpPlain special inv (chain, {'small' if self.small(2 * n * lp) else 'full'})", INV, (1, 1, 2 * n), 2))
        return out + [("OpModDown fwd (chain)", MD, (1, lp, 2 * n), 2)]

    def relinearize(self, a):
        return [x for n in self.chunks(a.batch) for x in self.key_switch(a.limbs, n)]

    def relinearize_many(self, cts):
        return self.key_switch(cts[0].limbs, len(cts))

    def relinearize_rescale(self, a, div):
        return [x for n in self.chunks(a.batch) for x in self.relin_rescale_core(a.limbs, n, False)]

    def relinearize_rescale_many(self, cts, div):
        return self.relin_rescale_core(cts[0].limbs, len(cts), False)

    def multiply_relinearize_rescale(self, a, b, div):
        if a.batch != 1 or b.batch != 1 or not self.fuse_mac:  # multiply (elementwise), then the batched call
            return [x for n in self.chunks(a.batch) for x in self.relin_rescale_core(a.limbs, n, False)]
        return self.relin_rescale_core(a.limbs, 1, True)

    def multiply_relinearize_rescale_many(self, cts_a, cts_b, div):
        return self.relin_rescale_core(cts_a[0].limbs, len(cts_a), self.fuse_mac)

    def multiply_rescale_relinearize_many(self, cts_a, cts_b, div):
        l, n = cts_a[0].limbs, len(cts_a) * cts_a[0].batch
        if self.chain_applies():
            return self.chain_step(l, n)
        return [("OpMulPolyIntt inv", INV, (1, 3 * n, 1), 1), ("OpModDownMul fwd", MD, (1, l - 1, 3 * n), 2)] + self.key_switch(l - 1, n)

    def multiply_rescale_relinearize(self, a, b, div):
        return self.multiply_rescale_relinearize_many([a], [b], div)

    def rescale_relinearize_many(self, cts, div):
        l, B = cts[0].limbs, cts[0].batch
        if self.chain_applies():
            return self.chain_step(l, len(cts) * B)
        out = []
        for _ in cts:  # the two calls per handle
            out += self.rescale_polys(l, 3 * B) + [x for n in self.chunks(B) for x in self.key_switch(l - 1, n)]
        return out

    def rescale_relinearize(self, a, div):
        return self.rescale_relinearize_many([a], div)

    def rescale_polys(self, l, polys):
        branch = "small" if self.small(polys * (l - 1)) else "full"
        return [(f"OpPlain last inv (rescale, {branch})", INV, (1, 1, polys), 2), (f"OpModDown fwd (rescale, {branch})", MD, (1, l - 1, polys), 2)]

    def rescale(self, a, div):
        return self.rescale_polys(a.limbs, a.size * a.batch)

    def rescale_many(self, cts, div):
        return self.rescale_polys(cts[0].limbs, len(cts) * cts[0].size)

    # ---- rotate.hip, rotation_sets.hip.h, windows.hip
    def hoist_wanted(self, l, n, B):
        return self.hoist and n >= 2 and self.N >= 2048 and n * B * l * (l + 1) * (self.N >> 11) >= self.hoist_min

    def sign_tables(self, steps):
        out = []
        for st in steps:
            elt = self.g.galois_elt_from_step(st)
            if elt not in self.signs:
                self.signs.add(elt)
                out.append(("OpPlain fwd (sign table)", NTT, (1, self.k, 1), 2))
        return out

    def hoist_digits(self, l, n_src):
        return [("OpPlainZ inv", INV, (1, l, n_src), 2), ("OpKsDigit fwd", KSD, (l, l + 1, n_src), 0)]

    def rot_mod_down(self, l, np_):
        branch = "small" if self.small(2 * np_ * l) else "full"
        return [(f"OpPlainG inv (rotation set, {branch})", INV, (1, 1, 2 * np_), 2), (f"OpModDownG fwd ({branch})", MD, (1, l, 2 * np_), 2)]

    def rotation_set(self, l, steps, B, n_src, chunk_pairs, hoisted):
        if not hoisted:
            return [x for np_ in chunk_pairs for x in self.key_switch(l, np_)]
        out = self.sign_tables(steps) + self.hoist_digits(l, n_src)
        return out + [x for np_ in chunk_pairs for x in self.rot_mod_down(l, np_)]  # (the fallback is one persistent launch)

    def rotate_many(self, a, steps):
        l, B, n = a.limbs, a.batch, len(steps)
        m_max = max(1, KS_BATCH_MAX // B)
        chunk_pairs = [min(m_max, n - j0) * B for j0 in range(0, n, m_max)]
        return self.rotation_set(l, steps, B, B, chunk_pairs, self.hoist_wanted(l, n, B))

    def rotate(self, a, step):
        if step == 0:
            return []
        return self.rotate_many(a, [step]) if a.batch > 1 else self.key_switch(a.limbs, 1)

    def rotate_weighted_sums(self, windows):
        l, B = windows[0][0][0][0].limbs, windows[0][0][0][0].batch
        fusable, n_rot, distinct, units = self.win_fuse and self.fold_pa, 0, [], []
        for terms, weights in windows:
            rot = [(ct, st) for ct, st in terms if st != 0]
            ids = len(terms) - len(rot)
            for ct, _ in rot:
                if ct.h.value not in distinct:
                    distinct.append(ct.h.value)
            if len(weights) > 2 or ids > 1 or ids == len(terms):
                fusable = False
            n_rot += len(rot)
            units += [(len(rot), len(weights))] * B
        steps = [st for terms, _ in windows for _, st in terms if st != 0]
        fusable = fusable and len(distinct) * B <= KS_BATCH_MAX and self.hoist_wanted(l, n_rot, B)
        if not fusable:  # the rotations as launch sets, then elementwise sums
            if B == 1:
                out = []
                for i0 in range(0, len(steps), KS_BATCH_MAX):
                    n = min(KS_BATCH_MAX, len(steps) - i0)
                    out += self.rotation_set(l, steps[i0:i0 + n], 1, len(distinct), [n], len(distinct) < n and self.hoist_wanted(l, n, 1))
                return out
            assert len(distinct) == 1 and len(steps) <= KS_BATCH_MAX, "(all this module asks of the general form)"
            return self.rotate_many(windows[0][0][0][0], steps)
        out = self.sign_tables(steps) + self.hoist_digits(l, len(distinct) * B)
        chunk = None  # [units, pairs, sums]
        for count, F in units + [(None, None)]:
            if chunk and (count is None or chunk[2] != F or chunk[0] == WIN_MAX or chunk[1] + count > KS_BATCH_MAX):
                branch = "small" if self.small(2 * chunk[1] * l) else "full"
                out.append((f"OpPlainG inv (window, {branch})", INV, (1, 1, 2 * chunk[1]), 2))
                chunk = None
            if count is not None:
                chunk = chunk or [0, 0, F]
                chunk[0] += 1
                chunk[1] += count
        return out

    # ---- no transform
    def multiply(self, a, b):
        return []

    upload_ct = upload_ct_batch = upload_pt = upload_relin_key = upload_galois_key = lambda self, *a: []


class _Counted:
    """A context whose every call is held against the model: loop_stats() must grow by what loop_plan gives for the launches
    of that call.  close(must) also asks that the sites in `must` are among those that looped."""
    PASS = ("galois_elt_from_step", "ks_tail", "loop_stats", "sync", "N", "k", "primes", "profile", "profile_reset", "profile_get",
            "modup_variant")

    def __init__(self, g, knobs, must=()):
        self.g, self.model, self.knobs, self.must = g, _Model(g, knobs), knobs, set(must)
        self.looped, self.total = set(), [0] * 6

    def __getattr__(self, name):
        fn = getattr(self.g, name)
        if name in self.PASS:
            return fn
        launches_of = getattr(self.model, name)  # a call this module has no launch list for fails here

        def call(*args):
            launches = launches_of(*args)
            before = self.g.loop_stats()
            out = fn(*args)
            got = tuple(a - b for a, b in zip(self.g.loop_stats(), before))
            want, sites = plan_stats(launches, self.g.N, self.knobs)
            assert got == want, (f"{name}: loop_stats() grew by {got}, the launch rule gives {want} for "
                                 f"{[(s, e, loop_plan(e, ax, self.g.N, self.knobs)) for s, _, e, ax in launches]} under {self.knobs}")
            self.looped |= sites
            self.total = [t + x for t, x in zip(self.total, got)]
            return out

        return call

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):  # the context is closed whatever ended the block; the sites are asked for after a clean one
        if exc_type is None:
            self.close()
        else:
            self.g.close()

    def close(self):
        try:
            missing = self.must - self.looped
            assert not missing, f"sites that were to run in the looped kernel and did not: {sorted(missing)}; looped: {sorted(self.looped)}"
        finally:
            self.g.close()


def _counted(N, primes, knobs, must=()):
    """knobs None: a context with no knob set at all (not even _ctx's EVAH_HOIST_MIN_TILES=0)"""
    if knobs is None:
        return _Counted(tge.backend.Context(N, primes), {}, must)
    knobs = dict({"EVAH_HOIST_MIN_TILES": 0}, **knobs)
    return _Counted(_ctx(N, primes, knobs), knobs, must)


@pytest.fixture
def counted():
    """_counted for tests that use one context for their whole body: whatever ends the test, the context is closed"""
    made = []

    def make(*args):
        made.append(_counted(*args))
        return made[-1]

    yield make
    for g in made:
        g.g.close()


# ---- (a) every pass size, both butterfly forms, worst-case words, every site
FORMS = {
    "default": {},
    "nosmall": {"EVAH_FUSE_SMALL": 0},
    "two_launch": {"EVAH_FUSE_SMALL": 0, "EVAH_MODUP": 0},
    "unfused": {"EVAH_FUSE_MAC": 0},
    "fold_pa0": {"EVAH_FOLD_PA": 0},
    "tail6": {"EVAH_FUSE_SMALL": 0, "EVAH_TAIL_FUSE": 0},
    "chain0": {"EVAH_CHAIN_STEP": 0},
    "special_inv0": {"EVAH_FUSE_SPECIAL_INV": 0},
}
HOISTED = {"OpKsDigit fwd"}  # (OpPlainZ's launch has one job per source: the zero-record test loops it)
# the sites each form is there for, at N >= 2048 (the docstring's table)
MUST = {
    "default": {"OpPlain digits inv (pass1)", "OpMulIntt+d2 inv (pass1)", "OpPlain special inv (tail)", "OpRRLastFolded inv", "OpRRFolded fwd",
                "OpChainIntt inv", "OpModDown fwd (chain)", "OpPlainG inv (window, small)", "OpPlainG inv (rotation set, small)",
                "OpModDownG fwd (small)", "OpModDown fwd (mod-down, small)"} | HOISTED,
    "nosmall": {"OpPlain digits inv (pass1)", "OpMulIntt+d2 inv (pass1)", "OpTailIntt inv", "OpRRFolded fwd (three)", "OpChainIntt inv",
                "OpPlain special inv (chain, full)", "OpModDown fwd (chain)", "OpPlainG inv (window, full)",
                "OpPlainG inv (rotation set, full)", "OpModDownG fwd (full)", "OpPlain special inv (mod-down, full)",
                "OpModDown fwd (mod-down, full)"} | HOISTED,
    "two_launch": {"OpPlain digits inv (both passes)", "OpMulIntt+d2 inv (both passes)", "OpPlain special inv (tail)", "OpRRLastFolded inv",
                   "OpRRFolded fwd"},
    "unfused": {"OpPlain digits inv (both passes)", "OpKsDigit fwd", "OpRRLast inv", "OpRR fwd", "OpMulPolyIntt inv", "OpModDownMul fwd"},
    "fold_pa0": {"OpMulIntt inv (pass1)", "OpRRLastMul inv", "OpRRMul fwd", "OpRRLast inv", "OpRR fwd", "OpMulPolyIntt inv", "OpModDownMul fwd"},
    "tail6": {"OpPlain special inv (tail)", "OpRRLastFolded inv", "OpRRFolded fwd"},
    "chain0": {"OpMulPolyIntt inv", "OpModDownMul fwd"},
    "special_inv0": {"OpChainIntt inv", "OpPlain special inv (chain, small)", "OpModDown fwd (chain)", "OpPlain special inv (mod-down, small)"},
}
# N = 1024: no small-launch form, no mod-up, no chain step, no hoisting — what is left of each form
MUST_1024 = {
    "default": {"OpPlain digits inv (both passes)", "OpMulIntt+d2 inv (both passes)", "OpPlain special inv (tail)", "OpRRLastFolded inv",
                "OpRRFolded fwd", "OpMulPolyIntt inv", "OpModDownMul fwd", "OpPlain special inv (mod-down, full)",
                "OpModDown fwd (mod-down, full)", "OpPlain last inv (rescale, full)", "OpModDown fwd (rescale, full)"},
    "unfused": {"OpPlain digits inv (both passes)", "OpKsDigit fwd", "OpRRLast inv", "OpRR fwd", "OpMulPolyIntt inv", "OpModDownMul fwd"},
    "fold_pa0": {"OpMulIntt inv (both passes)", "OpRRLastMul inv", "OpRRMul fwd", "OpRRLast inv", "OpRR fwd"},
}
CHAINS = {"c60": [60] * 4, "bits30_40": [40, 30, 40, 30, 40]}


def _site_cases():
    out = []
    for logN in (10, 11, 12, 14, 16):
        for chain in CHAINS:
            # 2^11 shares P_b = 5 with 2^10 and has what 2^10 lacks: the mod-up and tail kernels, the chain step, hoisting
            for form in (MUST_1024 if logN == 10 else ("default", "nosmall", "special_inv0") if logN == 11 else FORMS):
                out.append((f"N{1 << logN}-{chain}-{form}", logN, chain, form))
    return out


SITE_CASES = _site_cases()


@pytest.fixture(scope="module", autouse=True)
def _drop_the_oracle_words_after_the_module():
    """(_oracle is test_gpu_extremes_degrees.py's: one memo at a time, so the cases of one (degree, chain) stand together)"""
    yield
    _ORACLE.clear()
    _WALK.clear()


def _random_poly(primes, nl, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, primes[i], size=N, dtype=np.uint64) for i in range(nl)])


@pytest.mark.parametrize("name,logN,chain,form", SITE_CASES, ids=[c[0] for c in SITE_CASES])
def test_sites_loop_on_worst_case_words(name, logN, chain, form):
    """_check_key_switches (keys at q - 1; single, _many and batched calls of every key-switch form) with every contiguous
    launch of two or more jobs in the looped kernel; the counters are checked call by call, the sites at close().  Then
    the same on a second context with the keys at q - 1 mixed with zeros, on the dense_max and random words: what keys of
    -1 cannot show (module docstring)"""
    N = 1 << logN
    primes = po.coeff_modulus_create(N, CHAINS[chain])
    o = _oracle(N, primes)
    l = len(primes) - 1
    words = _forms(o, primes, l, N)
    if logN >= 16:
        words = [w for w in words if w[0] in ("qm1", "dense_max")]
    if chain == "c60":
        words.append(("searched", _searched_form(o, primes, N)))
    words.append(("random", _random_poly(primes, l, N, 11)))
    knobs = dict(FORCE, **FORMS[form])
    must = (MUST_1024 if logN == 10 else MUST)[form]
    for kind, some in (("qm1", words), ("mixed", [w for w in words if w[0] in ("dense_max", "random")])):
        try:
            with _counted(N, primes, knobs, must) as g:
                _check_key_switches(g, o, primes, np.random.default_rng(5), kind, forms=some)
        except AssertionError as e:
            raise AssertionError(f"N=2^{logN} chain {chain} form {form} keys {kind}: {e}") from e
        finally:
            o.forget_arrays()


TIE_FORMS = ["default", "nosmall", "unfused", "fold_pa0", "chain0"]
# the sites of the rescale and mod-down paths the tie words go through (single calls and one rescale_many of two)
TIE_MUST = {
    "default": {"OpPlain last inv (rescale, small)", "OpModDown fwd (rescale, small)", "OpRRLastFolded inv", "OpRRFolded fwd",
                "OpModDown fwd (chain)", "OpModDown fwd (mod-down, small)"},
    "nosmall": {"OpPlain last inv (rescale, full)", "OpModDown fwd (rescale, full)", "OpTailIntt inv", "OpRRFolded fwd (three)",
                "OpModDown fwd (chain)", "OpModDown fwd (mod-down, full)"},
    "unfused": {"OpRRLast inv", "OpRR fwd", "OpMulPolyIntt inv", "OpModDownMul fwd"},
    "fold_pa0": {"OpRRLastMul inv", "OpRRMul fwd", "OpRRLast inv", "OpRR fwd", "OpMulPolyIntt inv", "OpModDownMul fwd"},
    "chain0": {"OpMulPolyIntt inv", "OpModDownMul fwd"},
}
TIE_MUST_1024 = {
    "default": {"OpPlain last inv (rescale, full)", "OpModDown fwd (rescale, full)", "OpRRLastFolded inv", "OpRRFolded fwd",
                "OpMulPolyIntt inv", "OpModDownMul fwd", "OpModDown fwd (mod-down, full)"},
    "unfused": TIE_MUST["unfused"],
    "fold_pa0": TIE_MUST["fold_pa0"],
}


def _tie_cases():
    return [(f"N{1 << logN}-{chain}-{form}", logN, chain, form) for logN in (10, 12, 14, 16) for chain in CHAINS
            for form in (TIE_MUST_1024 if logN == 10 else TIE_FORMS)]


TIE_CASES = _tie_cases()


@pytest.mark.parametrize("name,logN,chain,form", TIE_CASES, ids=[c[0] for c in TIE_CASES])
def test_rounding_ties_loop(name, logN, chain, form, monkeypatch):
    """_check_rounding_ties (the dropped limb at 0, (q_last -+ 1) / 2, q_last - 1 through rescale, the fused forms, the
    chain step and the mod-down) on a counted context under the forcing knobs"""
    knobs = dict(FORCE, **FORMS[form])
    made = []

    def counted_ctx(N, primes, _):
        made.append(_counted(N, primes, knobs, (TIE_MUST_1024 if logN == 10 else TIE_MUST)[form]))
        return made[-1]

    monkeypatch.setattr(tge, "_ctx", counted_ctx)
    _check_rounding_ties(1 << logN, CHAINS[chain])
    assert len(made) == 1 and made[0].g.h is None, "the check ran on the counted context and closed it"


# ---- (b) walk shapes
_WALK = {}


def _walk_words(N, bits, B):
    """B instances that all hold different words (a hook applied to the wrong job of a walk shows), with what the oracle
    makes of them; computed once per (N, chain, B) and shared by the knob settings"""
    key = (N, tuple(bits), B)
    if key in _WALK:
        return _WALK[key]
    primes = po.coeff_modulus_create(N, bits)
    o = po.Oracle(N, primes)
    l = len(primes) - 1
    rng = np.random.default_rng(100 * B + l)
    rk = _keys(primes, l, N, rng, "mixed")  # not q - 1 everywhere: such a key hides a wrong digit set behind the rescale
    steps = [1, -3]
    gks = {st: _keys(primes, l, N, rng, "mixed") for st in steps}
    worst = dict(_forms(o, primes, l, N))
    polys = [worst["dense_max"], _random_poly(primes, l, N, 1), worst["qm1"], _random_poly(primes, l, N, 2), _ties(o, primes, l, N),
             _random_poly(primes, l, N, 3), worst["dense"]]
    pick = lambda i: polys[i % len(polys)]  # noqa: E731
    # instance b: a size-3 ciphertext and two size-2 ones, no two polynomials of an instance or of neighbours alike
    a3 = [np.stack([pick(3 * b), pick(3 * b + 1), pick(3 * b + 2)]) for b in range(B)]
    a2 = [np.stack([pick(2 * b + 1), pick(2 * b + 3)]) for b in range(2 * B)]
    w = {"primes": primes, "rk": rk, "gks": gks, "steps": steps, "a3": a3, "a2": a2, "l": l}
    relin = [o.relinearize(x, rk) for x in a3]
    w["relin"] = relin
    w["relin_rescale"] = [o.rescale(x) for x in relin]
    w["rescale3"] = [o.rescale(x) for x in a3]
    w["rescale2"] = [o.rescale(x) for x in a2]
    w["rescale_relin"] = [o.relinearize(x, rk) for x in w["rescale3"]]
    prod = [o.multiply(a2[i], a2[(i + 1) % (2 * B)]) for i in range(2 * B)]  # pair i: instance i times its neighbour
    w["triple"] = [o.rescale(o.relinearize(m, rk)) for m in prod]
    w["chain"] = [o.relinearize(o.rescale(m), rk) for m in prod]
    w["rot"] = [{st: o.rotate(x, st, gks[st]) for st in steps} for x in a2[:B]]
    wts = [_random_poly(primes, l, N, 20 + i) for i in range(3)]
    w["wts"] = wts
    w["window"] = []
    for b in range(B):
        acc = o.multiply_plain(a2[b], wts[0])
        for st, wt in zip(steps, wts[1:]):
            acc = o.add(acc, o.multiply_plain(w["rot"][b][st], wt))
        w["window"].append(acc)
    _WALK[key] = w
    return w


def _inst(got, b, B):
    return got[b] if B > 1 else got


def _check_walks(g, w, B):
    """relinearize (+ rescale) and the two fused products, rescale, rotations and a window on a batched handle of B
    instances (a single ciphertext for B = 1), and the _many calls on 2 B entries: instance b against the oracle's b"""
    g.upload_relin_key(w["rk"])
    for st in w["steps"]:
        g.upload_galois_key(g.galois_elt_from_step(st), w["gks"][st])
    div = int(w["primes"][w["l"] - 1]).bit_length()
    a3, a2 = w["a3"], w["a2"]
    up = (lambda xs: g.upload_ct_batch(np.stack(xs), 2.0 ** 20)) if B > 1 else (lambda xs: g.upload_ct(xs[0], 2.0 ** 20))
    H3, H2, H2n = up(a3), up(a2[:B]), up(a2[1:B + 1])
    singles = [g.upload_ct(x, 2.0 ** 20) for x in a2]
    n2 = len(singles)
    got = g.relinearize(H3).download()
    for b in range(B):
        _same(_inst(got, b, B), w["relin"][b], f"relinearize instance {b}")
    got = g.relinearize_rescale(H3, div).download()
    for b in range(B):
        _same(_inst(got, b, B), w["relin_rescale"][b], f"relinearize_rescale instance {b}")
    got = g.rescale_relinearize(H3, div).download()
    for b in range(B):
        _same(_inst(got, b, B), w["rescale_relin"][b], f"rescale_relinearize instance {b}")
    for H, want, what in ((H3, w["rescale3"], "size 3"), (H2, w["rescale2"], "size 2")):
        got = g.rescale(H, div).download()
        for b in range(B):
            _same(_inst(got, b, B), want[b], f"rescale {what} instance {b}")
    # the products of instance b and its neighbour: one batched handle against the handle shifted by one instance
    got = g.multiply_relinearize_rescale(H2, H2n, div).download()
    for b in range(B):
        _same(_inst(got, b, B), w["triple"][b], f"multiply_relinearize_rescale instance {b}")
    got = g.multiply_rescale_relinearize(H2, H2n, div).download()
    for b in range(B):
        _same(_inst(got, b, B), w["chain"][b], f"multiply_rescale_relinearize instance {b}")
    # 2 B different products in one launch set: OpMulIntt's first job through load, the later ones through raw_load / finish_load
    nxt = singles[1:] + singles[:1]
    for i, got in enumerate(g.multiply_relinearize_rescale_many(singles, nxt, div)):
        _same(got.download(), w["triple"][i], f"multiply_relinearize_rescale_many entry {i} of {n2}")
    for i, got in enumerate(g.multiply_rescale_relinearize_many(singles, nxt, div)):
        _same(got.download(), w["chain"][i], f"multiply_rescale_relinearize_many entry {i} of {n2}")
    for i, got in enumerate(g.rescale_many(singles, div)):
        _same(got.download(), w["rescale2"][i], f"rescale_many entry {i} of {n2}")
    for st, got in zip(w["steps"], g.rotate_many(H2, w["steps"])):
        got = got.download()
        for b in range(B):
            _same(_inst(got, b, B), w["rot"][b][st], f"rotate_many step {st} instance {b}")
    W = [g.upload_pt(x, 2.0 ** 10) for x in w["wts"]]
    got = g.rotate_weighted_sums([([(H2, st) for st in [0] + w["steps"]], [W])])[0].download()
    for b in range(B):
        _same(_inst(got, b, B), w["window"][b], f"rotate_weighted_sums instance {b}")


WALK_FORMS = {
    "default": {"OpMulIntt+d2 inv (pass1)", "OpRRFolded fwd", "OpModDown fwd (chain)", "OpModDown fwd (rescale, small)", "OpPlainG inv (window, small)"},
    "nosmall": {"OpMulIntt+d2 inv (pass1)", "OpRRFolded fwd (three)", "OpTailIntt inv", "OpModDown fwd (chain)", "OpModDown fwd (rescale, full)"},
    "fold_pa0": {"OpMulIntt inv (pass1)", "OpRRMul fwd", "OpRR fwd", "OpModDownMul fwd"},
}
WALK_CASES = [(4096, B, n) for B in (1, 2, 3) for n in (2, 3, 4, 5, 8)] + [(16384, 3, 4), (16384, 3, 5)]


@pytest.mark.parametrize("N,B,loop_n", WALK_CASES, ids=[f"N{N}-B{B}-loop_n{n}" for N, B, n in WALK_CASES])
def test_walks_along_polynomials_and_instances(N, B, loop_n):
    """loop axis 2: walks of EVAH_LOOP_N jobs over counts of B, 2 B and 3 B (and 4 B, 6 B in the _many calls), every job with
    words of its own; the hooks (OpMulIntt's Raw, OpRRT's LoopPre, OpModDownT's Pre) in the forms that run them"""
    w = _walk_words(N, [60] * 4, B)
    for form, must in WALK_FORMS.items():
        try:
            with _counted(N, w["primes"], dict(FORCE, EVAH_LOOP_N=loop_n, **FORMS[form]), must) as g:
                _check_walks(g, w, B)
        except AssertionError as e:
            raise AssertionError(f"form {form}: {e}") from e


DIGIT_CASES = [(4096, 2), (4096, 3), (4096, 8), (16384, 2)]


@pytest.mark.parametrize("N,loop_n", DIGIT_CASES, ids=[f"N{N}-loop_n{n}" for N, n in DIGIT_CASES])
def test_walks_along_digits_with_skipped_jobs(N, loop_n, counted):
    """loop axis 0 (OpKsDigit, EVAH_FUSE_MAC=0) at l = 5: output limb I has no job at digit I.  EVAH_LOOP_N=2 walks {0,1},
    {2,3}, {4}: limb 0 skips the first job of a walk, limb 1 the last of one, limb 4 a whole walk; 3 walks {0,1,2}, {3,4}:
    limb 2 skips the last of three; 8: one walk; the special row skips nothing.  Every digit holds different words."""
    bits = [60] * 6
    primes = po.coeff_modulus_create(N, bits)
    o = po.Oracle(N, primes)
    l = len(primes) - 1
    rng = np.random.default_rng(31)
    rk, gk = _keys(primes, l, N, rng, "mixed"), {st: _keys(primes, l, N, rng, "mixed") for st in (1, -3)}
    worst = dict(_forms(o, primes, l, N))
    g = counted(N, primes, dict(FORCE, EVAH_LOOP_N=loop_n, EVAH_FUSE_MAC=0), {"OpKsDigit fwd", "OpPlain digits inv (both passes)"})
    g.upload_relin_key(rk)
    for st, key in gk.items():
        g.upload_galois_key(g.galois_elt_from_step(st), key)
    div = 60
    cts = [np.stack([_random_poly(primes, l, N, 40 + i), worst["dense_max"], _random_poly(primes, l, N, 50 + i)]) for i in range(2)]
    H = [g.upload_ct(x, 2.0 ** 20) for x in cts]
    want = [o.relinearize(x, rk) for x in cts]
    for i in range(2):
        _same(g.relinearize(H[i]).download(), want[i], f"relinearize {i}")
        _same(g.relinearize_rescale(H[i], div).download(), o.rescale(want[i]), f"relinearize_rescale {i}")
    for i, got in enumerate(g.relinearize_rescale_many(H, div)):  # two instances with digits of their own: grid.z = 2
        _same(got.download(), o.rescale(want[i]), f"relinearize_rescale_many entry {i}")
    a2 = cts[0][1:]
    A2 = g.upload_ct(a2, 2.0 ** 20)
    _same(g.rotate(A2, 1).download(), o.rotate(a2, 1, gk[1]), "rotate")
    for st, got in zip((1, -3), g.rotate_many(A2, [1, -3])):  # the hoisted set's digit transforms
        _same(got.download(), o.rotate(a2, st, gk[st]), f"rotate_many step {st}")
    g.close()


def test_one_job_walks_under_loop_min_1():
    """EVAH_LOOP_MIN=1 (not clamped): launches of ONE job along the loop axis run in the looped kernel too, nloop = 1, a
    single job and nothing to prefetch — the single calls of _check_walks, whose digits' launch has grid (1, l, 1)"""
    w = _walk_words(4096, [60] * 4, 1)
    for form, site in (("default", "OpPlain digits inv (pass1)"), ("two_launch", "OpPlain digits inv (both passes)")):
        knobs = dict(FORCE, EVAH_LOOP_MIN=1, **FORMS[form])
        assert loop_plan((1, w["l"], 1), 2, 4096, knobs) == (1, 1)
        with _counted(4096, w["primes"], knobs, {site, "OpPlain fwd (sign table)", "OpPlainZ inv"}) as g:
            _check_walks(g, w, 1)


@pytest.mark.parametrize("loop_n", [7, 5], ids=["loop_n7", "loop_n5"])
def test_the_halving_rule(loop_n, counted):
    """EVAH_LOOP_TARGET_WGS at its default: a launch of count = 6 at N = 4096 is far from 8192 workgroups, so nloop
    (min(7, 6) = 6 -> 3 -> 2, and 5 -> 3 -> 2) halves down to 2 and the launch has three walks, which is what the walks
    counter must say"""
    w = _walk_words(4096, [60] * 4, 3)
    knobs = {"EVAH_LOOP_MIN_WGS": 0, "EVAH_LOOP_N": loop_n}
    assert loop_plan((1, 2, 6), 2, 4096, knobs) == (6, 2) and loop_plan((1, 2, 6), 2, 4096, dict(knobs, EVAH_LOOP_TARGET_WGS=0)) == (6, min(loop_n, 6))
    g = counted(4096, w["primes"], knobs)
    div = int(w["primes"][w["l"] - 1]).bit_length()
    H2 = g.upload_ct_batch(np.stack(w["a2"][:3]), 2.0 ** 20)
    before = g.loop_stats()
    got = g.rescale(H2, div).download()  # inverse (1, 1, 6), forward (1, 2, 6): two launches of 6 jobs in 3 walks each
    assert tuple(a - b for a, b in zip(g.loop_stats(), before)) == (1, 0, 0, 1, 12, 6)
    for b in range(3):
        _same(got[b], w["rescale2"][b], f"rescale instance {b}")
    _check_walks(g, w, 3)
    g.close()


# ---- (c) the zero-coefficient record under the looped inverse pass
def _with_zeros(o, primes, rng, a2, spec):
    a2 = a2.copy()
    for limb, count in spec:
        x = rng.integers(1, primes[limb], size=o.N, dtype=np.uint64)
        x[rng.choice(o.N, size=count, replace=False)] = 0
        a2[1][limb] = o.ntt(limb, x)
    return a2


ZERO_CASES = [(N, bits, case) for N, bits in ((4096, [60, 20, 60, 60]), (16384, [60, 20, 60, 60, 60, 60]))
              for case in ("several_zeros", "one_zero_flipped", "batched")] + [(2048, [40, 20, 40, 41], "batched"), (65536, [60] * 4, "batched")]


@pytest.mark.parametrize("N,bits,case", ZERO_CASES, ids=[f"N{N}-{case}" for N, _, case in ZERO_CASES])
def test_zero_coefficient_record_under_the_looped_inverse_pass(N, bits, case, counted):
    """test_gpu_hoist.py's zero-coefficient cases with OpPlainZ's contiguous pass, whose first workgroup clears the record
    (first_pass_clear), in the looped kernel; the recording runs a launch later.  Each set runs twice around a set without
    zeros on the same context: a record that was not cleared shows in the calls after the first."""
    primes = po.coeff_modulus_create(N, bits)
    o = po.Oracle(N, primes)
    k, l = len(primes), len(primes) - 1
    rng = np.random.default_rng(7 * N + l)
    steps = [1, 65, -3]
    keys = {st: np.stack([np.stack([_random_poly(primes, k, N, 1000 + 10 * st + 2 * j + p) for p in range(2)]) for j in range(l)]) for st in steps}
    # a single ciphertext's OpPlainZ launch has one job per limb: it loops under EVAH_LOOP_MIN=1
    knobs = dict(FORCE) if case == "batched" else dict(FORCE, EVAH_LOOP_MIN=1)
    g = counted(N, primes, knobs, {"OpPlainZ inv"})
    for st in steps:
        g.upload_galois_key(g.galois_elt_from_step(st), keys[st])
    rand = lambda seed: np.stack([_random_poly(primes, l, N, seed), _random_poly(primes, l, N, seed + 1)])  # noqa: E731
    several = ((0, 5), (min(2, l - 2), 3), (l - 1, 1))
    if case == "batched":
        nb = 6 if N < 65536 else 2  # (two instances are a walk already; the oracle's rotations at 2^16 take a second each)
        inst = [rand(60 + 2 * b) for b in range(nb)]
        for b, spec in ((1, ((0, 2),)), (nb - 2, ((1, 1), (l - 1, 2)))):
            inst[b] = _with_zeros(o, primes, rng, inst[b], spec)
        sets = [inst, [rand(80 + 2 * b) for b in range(nb)], inst]
    else:
        if case == "several_zeros":
            a2 = _with_zeros(o, primes, rng, rand(60), several)
        else:  # one zero, at a position whose image under the first rotation is sign-flipped
            elt = po.galois_elt_from_step(N, steps[0])
            kpos = next(i for i in range(1, N) if ((i * elt) >> (N.bit_length() - 1)) & 1)
            x = rng.integers(1, primes[0], size=N, dtype=np.uint64)
            x[kpos] = 0
            a2 = rand(60)
            a2[1][0] = o.ntt(0, x)
        sets = [[a2], [rand(90)], [a2]]
    want = {}
    for run, insts in enumerate(sets):
        H = g.upload_ct_batch(np.stack(insts), 2.0 ** 20) if len(insts) > 1 else g.upload_ct(insts[0], 2.0 ** 20)
        for st, got in zip(steps, g.rotate_many(H, steps)):
            got = got.download()
            for b, a in enumerate(insts):
                key = (hashlib.blake2b(a.data, digest_size=16).digest(), st)
                if key not in want:
                    want[key] = o.rotate(a, st, keys[st])
                _same(_inst(got, b, len(insts)), want[key], f"{case}: run {run} step {st} instance {b}")
    g.close()


# ---- (d) the default gate, both sides, and the metric shape
def test_the_default_gate_at_the_benchmark_degree(counted):
    """No knobs.  At N = 65536 a rescale of a size-2 ciphertext has the forward combine (1, l - 1, 2): 256 (l - 1)
    workgroups at two jobs per walk, so l - 1 = 8 reaches EVAH_LOOP_MIN_WGS = 2048 and l - 1 = 7 does not; its inverse
    launch (1, 1, 2) never does.  The metric shape (l = 10): of one multiply_relinearize_rescale's three contiguous
    launches — OpMulIntt (1, 10, 1), OpTailIntt (1, 2, 2), OpRRFolded (1, 9, 2) — only the last is looped."""
    N, l = 65536, 10
    assert loop_plan((1, 8, 2), 2, N, {}) == (2, 2) and loop_plan((1, 7, 2), 2, N, {}) is None and loop_plan((1, 1, 2), 2, N, {}) is None
    assert loop_plan((1, 9, 2), 2, N, {}) == (2, 2) and loop_plan((1, 2, 2), 2, N, {}) is None and loop_plan((1, 10, 1), 2, N, {}) is None
    primes = po.coeff_modulus_create(N, [60] * (l + 1))
    o = po.Oracle(N, primes)
    g = counted(N, primes, None)
    rk = _keys(primes, l, N, np.random.default_rng(3), "mixed")
    g.upload_relin_key(rk)
    for nl, looped in ((9, (0, 0, 0, 1, 2, 1)), (8, (0, 0, 0, 0, 0, 0))):
        a2 = np.stack([_random_poly(primes, nl, N, 70 + nl), _ties(o, primes, nl, N)])
        A2 = g.upload_ct(a2, 2.0 ** 20)
        before = g.loop_stats()
        got = g.rescale(A2, 60).download()
        assert tuple(a - b for a, b in zip(g.loop_stats(), before)) == looped, f"rescale at l = {nl}"
        _same(got, o.rescale(a2), f"rescale at l = {nl}")
    a2 = np.stack([_random_poly(primes, l, N, 81), _random_poly(primes, l, N, 82)])
    b2 = np.stack([_random_poly(primes, l, N, 83), np.stack([np.full(N, primes[i] - 1, dtype=np.uint64) for i in range(l)])])
    A2, B2 = g.upload_ct(a2, 2.0 ** 20), g.upload_ct(b2, 2.0 ** 20)
    before = g.loop_stats()
    got = g.multiply_relinearize_rescale(A2, B2, 60).download()
    assert tuple(a - b for a, b in zip(g.loop_stats(), before)) == (0, 0, 0, 1, 2, 1), "the metric shape's looped launches"
    assert g.looped >= {"OpRRFolded fwd (three)", "OpModDown fwd (rescale, small)"}
    _same(got, o.rescale(o.relinearize(o.multiply(a2, b2), rk)), "multiply_relinearize_rescale at the metric shape")
    g.close()
