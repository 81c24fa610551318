"""Seed-compressed evaluation keys on the MI355X: what the seeds save from keygen to the first execute().

  python scripts/key_upload_probe.py harris --compress 0|1 [--uploads K]
      One key pair with the Harris rotation set (BASELINE config 3: N = 2^15, 9 primes, relinearization key + one
      Galois key per rotation step).
  python scripts/key_upload_probe.py relin --compress 0|1 [--uploads K]
      The relinearization key alone at N = 2^16, k = 11 (115 MB in full).

Each run prints one line: host time of generate_keys, bytes of the saved context, wall time of uploading the whole key
set through the C ABI on a fresh context (evah_key_upload or evah_key_upload_seeded; median of K uploads, each replacing
the keys of the one before), and — harris — the wall time of the first execute(), which creates the device state and
uploads the keys before it walks the program.  --compress 0 is the baseline: the same probe on full keys.

Device time of the expansion kernel: run one compressed leg under the profiler, which this script never starts itself,

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/key_upload_probe.py relin --compress 1 --uploads 20

and read the median duration of k_key_expand from the kernel trace (scripts/rocprof_summary.py).
"""
import argparse
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("what", choices=["harris", "relin"])
ap.add_argument("--compress", type=int, choices=[0, 1], default=1)
ap.add_argument("--uploads", type=int, default=5)
args = ap.parse_args()

import numpy as np
from eva import save
from eva.ckks import CKKSParameters
from eva.seal import generate_keys
from eva_amd import backend, workloads

compress = bool(args.compress)
if args.what == "harris":
    compiled, params, sig, inputs = workloads.compile_config("c3")
else:
    compiled, params = None, CKKSParameters([60] + [50] * 9 + [60], set(), 1 << 16)

t0 = time.perf_counter()
pub, sec = generate_keys(params, 1, compress_keys=compress)
t_keygen = time.perf_counter() - t0
assert pub.keys_compressed == compress

with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "ctx.sealpub")
    save(pub, path)
    file_bytes = os.path.getsize(path)

# the key set through the C ABI, as HipPublic::upload_eval_keys sends it
N, primes = pub.poly_modulus_degree, pub.primes
words = {0: pub.relin_key()}
words.update(pub.galois_keys())
seeds = pub.key_seeds()
c0 = {e: np.ascontiguousarray(w[:, 0]) for e, w in words.items()} if compress else None
sent = sum((c0[e].nbytes + seeds[e].nbytes) if compress else w.nbytes for e, w in words.items())
ctx = backend.Context(N, primes, device=0)
t = []
for _ in range(args.uploads):
    t0 = time.perf_counter()
    for e, w in words.items():
        if compress:
            (ctx.upload_relin_key_seeded(c0[e], seeds[e]) if e == 0 else ctx.upload_galois_key_seeded(e, c0[e], seeds[e]))
        else:
            (ctx.upload_relin_key(w) if e == 0 else ctx.upload_galois_key(e, w))
    t.append(time.perf_counter() - t0)
t.sort()
hbm = ctx.key_bytes_detail()
ctx.close()
n_keys = len(words)
del words, c0

line = (f"{args.what} compress_keys={int(compress)}: N={N} k={len(primes)} keys={n_keys} "
        f"generate_keys {t_keygen:.3f} s; saved context {file_bytes} bytes; key upload {sent} bytes h2d, "
        f"median {t[len(t) // 2] * 1e3:.2f} ms, min {t[0] * 1e3:.2f} ms over {len(t)} uploads; HBM (words, split, perm) {hbm}")
if compiled is not None:
    enc = pub.encrypt(inputs, sig)
    pub.synchronize()
    t0 = time.perf_counter()
    pub.execute(compiled, enc)
    pub.synchronize()
    line += f"; first execute() {(time.perf_counter() - t0) * 1e3:.2f} ms"
print(line)
