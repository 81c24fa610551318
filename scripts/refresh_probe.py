#!/usr/bin/env python
"""Refresh against the path that existed before it (DESIGN.md 1.12 *Measured*), on one box in one session.

    PYTHONPATH=. python scripts/refresh_probe.py [--out DIR] [--no-trace]

For each shape a batch of values at a low level is brought back to the top of the chain at the same scale, two ways:
  refresh   secret_ctx.refresh(batch, signature)
  dec->enc  secret_ctx.decrypt_array(batch, device=True) -> secret_ctx.encrypt_array(the DeviceArray): the decoder's and
            the encoder's FP64 special FFTs, the encodability sums and a host wait per array
Shapes: BASELINE config 4's (256 values, N = 2^14, 6 primes) and config 3's (64 values, N = 2^15, 9 primes), 4096 slots
used.  Host clock around calls that end in a device synchronise; medians of 7 after 2 warm-ups.  The driver starts every
GPU step as a child process under a time limit of its own and stops at the first that fails.  The last step runs one
shape under `rocprofv3 --kernel-trace` and reports the median duration of k_refresh_lift from the trace."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

SHAPES = {"c4": (256, 1 << 14, [60, 40, 40, 40, 40, 60]), "c3": (64, 1 << 15, [60] + [40] * 7 + [60])}
VEC, SCALE_BITS, LOW_LIMBS = 4096, 30, 2


def setup(shape):
    import numpy as np
    from eva.ckks import CKKSParameters, CKKSSignature, CKKSEncodingInfo
    from eva.seal import generate_keys
    from eva_amd._eva import Type
    B, N, bits = SHAPES[shape]
    k = len(bits)
    pub, sec = generate_keys(CKKSParameters(bits, set(), N), 5)
    low = CKKSSignature(VEC, {"x": CKKSEncodingInfo(Type.Cipher, SCALE_BITS, k - 1 - LOW_LIMBS)})
    top = CKKSSignature(VEC, {"x": CKKSEncodingInfo(Type.Cipher, SCALE_BITS, 0)})
    xs = np.random.default_rng(1).uniform(-1, 1, (B, VEC))
    return pub, sec, low, top, sec.encrypt_array({"x": xs}, low, seed=3), xs


def step_time(shape):
    import numpy as np
    pub, sec, low, top, vb, xs = setup(shape)

    def refresh():
        return sec.refresh(vb, top)

    def dec_enc():
        out = sec.encrypt_array(sec.decrypt_array(vb, low, device=True), top)
        pub.synchronize()
        return out

    res = {"shape": shape, "values": SHAPES[shape][0], "N": SHAPES[shape][1], "primes": len(SHAPES[shape][2])}
    for name, fn in (("refresh", refresh), ("dec_enc", dec_enc)):
        for _ in range(2):
            out = fn()
        ts = []
        for _ in range(7):
            pub.synchronize()
            t0 = time.perf_counter()
            out = fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        err = float(np.abs(sec.decrypt_array(out, top)["x"] - xs).max())
        res[name + "_ms_median"], res[name + "_ms_min"], res[name + "_ms_max"] = statistics.median(ts), min(ts), max(ts)
        res[name + "_max_error"] = err
    print(json.dumps(res), flush=True)


def step_once(shape):
    pub, sec, low, top, vb, _ = setup(shape)
    for _ in range(9):
        sec.refresh(vb, top)


def lift_durations(trace_dir):
    out = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if "k_refresh_lift" in row.get("Kernel_Name", ""):
                    out.append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", choices=["time", "once"], help="(a child of the driver) one GPU step")
    ap.add_argument("--shape", choices=list(SHAPES), default="c4")
    ap.add_argument("--out", default="refresh_probe_out")
    ap.add_argument("--no-trace", action="store_true")
    args = ap.parse_args()
    if args.step == "time":
        return step_time(args.shape)
    if args.step == "once":
        return step_once(args.shape)
    os.makedirs(args.out, exist_ok=True)
    me = [sys.executable, os.path.abspath(__file__)]
    steps = [(me + ["--step", "time", "--shape", s], 300) for s in SHAPES]
    trace_dir = os.path.join(args.out, "trace")
    if not args.no_trace:
        steps.append((["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", trace_dir, "--"] + me + ["--step", "once", "--shape", "c4"], 300))
    for cmd, limit in steps:
        print("+", " ".join(cmd), flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc:
            print(f"step failed (status {rc}): nothing more is started", flush=True)
            return rc
    if not args.no_trace:
        d = lift_durations(trace_dir)
        print(json.dumps({"kernel": "k_refresh_lift", "shape": "c4", "dispatches": len(d),
                          "us_median": statistics.median(d) if d else None, "us_min": min(d) if d else None, "us_max": max(d) if d else None}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
