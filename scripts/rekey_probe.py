#!/usr/bin/env python
"""Re-key against the path that existed before it (DESIGN.md 1.13 *Measured*), on one box in one session.

    PYTHONPATH=. python scripts/rekey_probe.py

For each shape a batch of values under key pair A is handed to key pair B on the same GPU, two ways:
  rekey     public_ctx_B.rekey(batch, rekey_key) — public material only
  dec->enc  secret_ctx_A.decrypt_array(batch, device=True) -> public_ctx_B.encrypt_array(the DeviceArray): needs A's
            secret key where it runs, and rounds through FP64 slots
Shapes: BASELINE config 4's (256 values, N = 2^14, 6 primes) and config 3's (64 values, N = 2^15, 9 primes), at the top of
the chain, 4096 slots used.  Host clock around calls that end in a device synchronise; medians of 7 after 2 warm-ups.
Then, per scale 2^30, 2^40 and 2^50 at config 4's shape: the largest slot difference between B's decryption of the
re-keyed batch and A's own decryption of its source.  The driver starts every GPU step as a child process under a time
limit of its own and stops at the first that fails.  No speed ratio is a goal: the value of rekey is that it needs no
secret key."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

SHAPES = {"c4": (256, 1 << 14, [60, 40, 40, 40, 40, 60]), "c3": (64, 1 << 15, [60] + [40] * 7 + [60])}
VEC = 4096


def setup(shape, scale_bits, values=None):
    import numpy as np
    from eva.ckks import CKKSParameters, CKKSSignature, CKKSEncodingInfo
    from eva.seal import generate_keys
    from eva_amd._eva import Type
    B, N, bits = SHAPES[shape]
    B = values or B
    params = CKKSParameters(bits, set(), N)
    (pub_a, sec_a), (pub_b, sec_b) = generate_keys(params, 5), generate_keys(params, 6)
    sig = CKKSSignature(VEC, {"x": CKKSEncodingInfo(Type.Cipher, scale_bits, 0)})
    xs = np.random.default_rng(1).uniform(-1, 1, (B, VEC))
    rk = sec_a.make_rekey_key(pub_b, seed=7)
    pub_b.install_rekey_key(rk)
    return pub_a, sec_a, pub_b, sec_b, sig, rk, pub_a.encrypt_array({"x": xs}, sig, seed=3), xs


def step_time(shape):
    import numpy as np
    pub_a, sec_a, pub_b, sec_b, sig, rk, vb, xs = setup(shape, 30)

    def rekey():
        out = pub_b.rekey(vb, rk)
        pub_b.synchronize()
        return out

    def dec_enc():
        out = pub_b.encrypt_array(sec_a.decrypt_array(vb, sig, device=True), sig)
        pub_b.synchronize()
        return out

    res = {"shape": shape, "values": SHAPES[shape][0], "N": SHAPES[shape][1], "primes": len(SHAPES[shape][2])}
    for name, fn in (("rekey", rekey), ("dec_enc", dec_enc)):
        for _ in range(2):
            out = fn()
        ts = []
        for _ in range(7):
            pub_a.synchronize()
            pub_b.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms_median"], res[name + "_ms_min"], res[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
        res[name + "_max_error"] = float(np.abs(sec_b.decrypt_array(out, sig)["x"] - xs).max())
    print(json.dumps(res), flush=True)


def step_precision(shape):
    import numpy as np
    for bits in (30, 40, 50):
        pub_a, sec_a, pub_b, sec_b, sig, rk, vb, xs = setup(shape, bits, values=64)
        ref = sec_a.decrypt_array(vb, sig)["x"]
        got = sec_b.decrypt_array(pub_b.rekey(vb, rk), sig)["x"]
        print(json.dumps({"shape": shape, "scale_bits": bits, "limbs": len(SHAPES[shape][2]) - 1,
                          "rekey_max_slot_difference": float(np.abs(got - ref).max()),
                          "source_max_error": float(np.abs(ref - xs).max())}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["time", "precision"], help="(a child of the driver) one GPU step")
    ap.add_argument("--shape", choices=list(SHAPES), default="c4")
    args = ap.parse_args()
    if args.step == "time":
        return step_time(args.shape)
    if args.step == "precision":
        return step_precision(args.shape)
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [(me + ["--step", "time", "--shape", s], 300) for s in SHAPES] + [(me + ["--step", "precision", "--shape", "c4"], 300)]
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
