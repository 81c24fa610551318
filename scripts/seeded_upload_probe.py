"""Seeded symmetric ciphertexts on the MI355X: what the seed saves on a host-valuation execute().

  python scripts/seeded_upload_probe.py harris public|seeded [--calls K]
      Harris (BASELINE config 3: N = 2^15, 9 primes) with host valuations (EVA_RESIDENT=0): K timed execute() calls
      on public-key or on seeded inputs, each on a fresh key pair; prints the median wall time per call and the h2d
      bytes of one call.  Run each kind under rocprofv3 --kernel-trace --memory-copy-trace --stats for device times.
  python scripts/seeded_upload_probe.py spans <rocpd results .db>
      From the kernel + memory-copy trace of a harris run: the device-side span of each execute() (start of its input
      copy to the end of its last copy or kernel), median and minimum over the last 50 calls.
  python scripts/seeded_upload_probe.py expand [--calls K]
      K seeded uploads of a [10][2^16] ciphertext (zero c0): the k_expand_seeded launches for a rocprofv3 kernel trace.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("what", choices=["harris", "expand", "spans"])
ap.add_argument("kind", nargs="?", default="seeded", help="harris: public | seeded; spans: the .db file")
ap.add_argument("--calls", type=int, default=50)
args = ap.parse_args()

if args.what == "spans":
    import collections
    import sqlite3
    import statistics
    db = sqlite3.connect(args.kind)
    ev = [(s, e) for s, e in db.execute("select start, end from kernels")]
    copies = db.execute("select start, end, src_agent_type, dst_agent_type, size from memory_copies").fetchall()
    ev += [(s, e) for s, e, _, _, _ in copies]
    h2d = [(s, sz) for s, _, a, b, sz in copies if a == "CPU" and b == "GPU"]
    # every execute() on host valuations starts with the copy of its ciphertext input: the most frequent h2d size
    size = collections.Counter(sz for _, sz in h2d).most_common(1)[0][0]
    starts = sorted(s for s, sz in h2d if sz == size)
    ev.sort()
    spans = []
    for a, b in zip(starts, starts[1:] + [float("inf")]):
        ends = [e for s, e in ev if a <= s < b]
        spans.append((max(ends) - a) / 1e6)
    last = spans[-50:]
    print(f"{len(spans)} calls (input copy {size} bytes): device span per execute() median {statistics.median(last):.3f} ms, "
          f"min {min(last):.3f} ms over the last {len(last)}")
    sys.exit(0)

if args.what == "expand":
    import numpy as np
    from eva_amd import backend
    from eva_amd.hostref import coeff_modulus_create
    N = 1 << 16
    primes = coeff_modulus_create(N, [60] + [50] * 10)
    ctx = backend.Context(N, primes, device=0)
    c0 = np.zeros((1, 10, N), dtype=np.uint64)
    t = []
    for i in range(args.calls):
        t0 = time.perf_counter()
        ct = ctx.upload_ct_seeded(c0, [bytes([i % 256]) * 32], 2.0 ** 40)
        t.append(time.perf_counter() - t0)
        ct.free()
    t.sort()
    print(f"seeded upload of [10][2^16] (c0 zero, synchronous): median {t[len(t) // 2] * 1e6:.1f} us wall")
    ctx.close()
    sys.exit(0)

os.environ["EVA_RESIDENT"] = "0"  # read when the key pair is made: host valuations
from eva.seal import generate_keys
from eva_amd import workloads

compiled, params, sig, inputs = workloads.compile_config("c3")
pub, sec = generate_keys(params, 1)
enc = sec.encrypt(inputs, sig, seed=1) if args.kind == "seeded" else pub.encrypt(inputs, sig)
for _ in range(5):  # eager walk, capture, replays
    pub.execute(compiled, enc)
pub.synchronize()
before = pub.transfer_stats()["h2d_bytes"]
pub.execute(compiled, enc)
h2d = pub.transfer_stats()["h2d_bytes"] - before
t = []
for _ in range(args.calls):
    t0 = time.perf_counter()
    pub.execute(compiled, enc)
    t.append(time.perf_counter() - t0)
t.sort()
print(f"harris {args.kind}: execute() median {t[len(t) // 2] * 1e3:.3f} ms, p10 {t[len(t) // 10] * 1e3:.3f} ms "
      f"over {args.calls} calls; h2d bytes per call {h2d}")
