#!/usr/bin/env python
"""The two rounds of the collective relinearization-key generation beside evah_keygen_rekey (DESIGN.md 1.15 *Measured*), on
one box in one session.

    PYTHONPATH=. python scripts/relin_rounds_probe.py

For each shape one party's calls at the C-ABI, with k - 1 digits:
  round1   evah_keygen_relin_round1   64 bytes per digit up, [D][2][k][N] down
  round2   evah_keygen_relin_round2   [D][2][k][N] + 64 bytes per digit up, [D][k][N] down
  rekey    evah_keygen_rekey          the yardstick, in the same process: [2][k][N] + 32 bytes per digit up, [D][2][k][N] down —
                                      the same class of bytes (sampling, one memory-bound kernel, a key-sized copy back)
Shapes: N = 2^14 with 6 primes and N = 2^15 with 9 primes.  Host clock around calls that end in their own drain; medians of
7 after 2 warm-ups.  The driver starts every shape as a child process under a time limit of its own and stops at the first
that fails.  The figures gate nothing."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

SHAPES = {"n14": (1 << 14, [60, 40, 40, 40, 40, 60]), "n15": (1 << 15, [60] + [40] * 7 + [60])}


def step(shape):
    import numpy as np
    from eva_amd import backend
    from eva_amd.hostref import coeff_modulus_create
    N, bits = SHAPES[shape]
    primes = coeff_modulus_create(N, bits)
    k, D = len(primes), len(primes) - 1
    rng = np.random.default_rng(N)

    def rand(prefix):
        return np.stack([rng.integers(0, primes[i], size=prefix + (N,), dtype=np.uint64) for i in range(k)], axis=len(prefix))

    def keys():
        return np.frombuffer(rng.bytes(32 * D), dtype=np.uint8).reshape(D, 32).copy()

    g = backend.Context(N, primes)
    try:
        g.upload_secret_key(rand(()))
        seeds, r1, r2, agg, pk = keys(), keys(), keys(), rand((D, 2)), rand((2,))
        calls = (("round1", lambda: g.keygen_relin_round1(seeds, r1)), ("round2", lambda: g.keygen_relin_round2(agg, r1, r2)),
                 ("rekey", lambda: g.keygen_rekey(pk, r1)))
        res = {"shape": shape, "N": N, "primes": k, "digits": D}
        for name, fn in calls:
            for _ in range(2):
                fn()
            ts = []
            for _ in range(7):
                t0 = time.perf_counter()
                out = fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            res[name + "_ms_median"], res[name + "_ms_min"], res[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
            res[name + "_bytes_down"] = int(out.nbytes)
        print(json.dumps(res), flush=True)
    finally:
        g.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shape", choices=list(SHAPES), help="(a child of the driver) one shape")
    args = ap.parse_args()
    if args.shape:
        return step(args.shape)
    me = [sys.executable, os.path.abspath(__file__)]
    for s in SHAPES:
        cmd = me + ["--shape", s]
        print("+", " ".join(cmd), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=300).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print(f"step failed (status {rc}): nothing more is started", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
