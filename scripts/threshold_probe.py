#!/usr/bin/env python
"""Threshold decryption against the decryption it replaces (DESIGN.md 1.14 *Measured*), on one box in one session.

    PYTHONPATH=. python scripts/threshold_probe.py

For each shape a batch of values under a collective key of three parties is opened two ways on the same GPU:
  share     one party's secret_ctx.decrypt_share(batch, 40)            (every party does this once)
  combine   public_ctx.combine_shares(batch, [3 shares], signature)    (once)
  decrypt   secret_ctx.decrypt_array(batch, signature) of the same values under one party's own key: the baseline
Shapes: BASELINE config 4's (256 values, N = 2^14, 6 primes) and config 3's (64 values, N = 2^15, 9 primes), at the top of
the chain, 4096 slots used.  Host clock around calls that end in a device synchronise; medians of 7 after 2 warm-ups.
--step kernels runs each call a few times and nothing else: the run a kernel trace is taken of.  The driver starts every
GPU step as a child process under a time limit of its own and stops at the first that fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

SHAPES = {"c4": (256, 1 << 14, [60, 40, 40, 40, 40, 60]), "c3": (64, 1 << 15, [60] + [40] * 7 + [60])}
VEC, SMUDGE, PARTIES = 4096, 40, 3


def setup(shape):
    import numpy as np
    from eva.ckks import CKKSParameters, CKKSSignature, CKKSEncodingInfo
    from eva.seal import combine_public_contexts, generate_keys
    from eva_amd._eva import Type
    B, N, bits = SHAPES[shape]
    params = CKKSParameters(bits, set(), N)
    pairs = [generate_keys(params, seed=5 + p, common_seed=bytes(32)) for p in range(PARTIES)]
    col = combine_public_contexts([pub for pub, _ in pairs])
    sig = CKKSSignature(VEC, {"x": CKKSEncodingInfo(Type.Cipher, 30, 0)})
    xs = np.random.default_rng(1).uniform(-1, 1, (B, VEC))
    return pairs, col, sig, col.encrypt_array({"x": xs}, sig, seed=3), pairs[0][0].encrypt_array({"x": xs}, sig, seed=3), xs


def timed(fn, sync):
    for _ in range(2):
        out = fn()
    ts = []
    for _ in range(7):
        sync()
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, {"ms_median": statistics.median(ts), "ms_min": min(ts), "ms_max": max(ts)}


def step_time(shape):
    import numpy as np
    pairs, col, sig, vb, own, xs = setup(shape)
    sec0 = pairs[0][1]
    shares = [sec.decrypt_share(vb, SMUDGE) for _, sec in pairs]
    res = {"shape": shape, "values": SHAPES[shape][0], "N": SHAPES[shape][1], "primes": len(SHAPES[shape][2]), "parties": PARTIES, "smudge_bits": SMUDGE}
    _, res["share"] = timed(lambda: sec0.decrypt_share(vb, SMUDGE), col.synchronize)
    got, res["combine"] = timed(lambda: col.combine_shares(vb, shares, sig)["x"], col.synchronize)
    ref, res["decrypt_array"] = timed(lambda: sec0.decrypt_array(own, sig)["x"], col.synchronize)
    res["combine_max_error"] = float(np.abs(got - xs).max())
    res["decrypt_max_error"] = float(np.abs(ref - xs).max())
    res["flood_bound"] = SHAPES[shape][1] * PARTIES * 2.0 ** SMUDGE / 2.0 ** 30
    print(json.dumps(res), flush=True)


def step_kernels(shape):
    pairs, col, sig, vb, own, xs = setup(shape)
    for _ in range(5):
        shares = [sec.decrypt_share(vb, SMUDGE) for _, sec in pairs]
        col.combine_shares(vb, shares, sig)
    col.synchronize()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["time", "kernels"], help="(a child of the driver) one GPU step")
    ap.add_argument("--shape", choices=list(SHAPES), default="c4")
    args = ap.parse_args()
    if args.step == "time":
        return step_time(args.shape)
    if args.step == "kernels":
        return step_kernels(args.shape)
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [(me + ["--step", "time", "--shape", s], 300) for s in SHAPES]
    for cmd, limit in steps:
        print("+", " ".join(cmd), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print(f"step failed (status {rc}): nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
