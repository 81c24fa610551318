"""Evaluation keys generated on the MI355X: what generate_keys costs with the keys made on the device.

  python scripts/keygen_probe.py relin --device 0|1
      The relinearization key alone at N = 2^16, k = 11 (10 digits, 57.7 MB of c0).
  python scripts/keygen_probe.py harris --device 0|1
      One key pair with the Harris rotation set (BASELINE config 3: N = 2^15, 9 primes, relinearization key + one
      Galois key per rotation step), then the first execute().

Each run prints one line: wall time of generate_keys, the bytes that crossed the host boundary during it
(transfer_stats: host -> device and device -> host), the bytes of evaluation-key words held on the host and the HBM bytes
of evaluation keys right after it, — harris — the wall time of the first execute(), which uploads the keys first when
they are not on the device yet, and the wall time of the first save(), which fetches c0 first when it is not on the host
yet.  --device 0 is the baseline: generate_keys(..., compress_keys=True) on the host, the path before this option, on the
same box.  The two legs produce the same keys for one seed (tests/test_gpu_keygen.py); --check compares them here as well.

  --sampling device    every polynomial of the key set from a 32-byte key: with --device 1 the whole set is
      one evah_keygen_public and one evah_keygen_set, with --device 0 the host twin computes the same keys.  --sampling
      host (the default) is the path above.  --warmup W generates W key pairs before the timed ones.

Device time of the kernel: run one --device 1 leg under the profiler, which this script never starts itself,

  rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/keygen_probe.py relin --device 1 --repeat 20

and read the median duration of k_keygen_switch (--sampling device: k_sample_small, k_keygen_set) from the kernel trace
(scripts/rocprof_summary.py).
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
ap.add_argument("--device", type=int, choices=[0, 1], default=1)
ap.add_argument("--repeat", type=int, default=1, help="key pairs generated (the median wall time is reported)")
ap.add_argument("--sampling", choices=["host", "device"], default="host", help="device: generate_keys(..., device_sampling=True)")
ap.add_argument("--warmup", type=int, default=0, help="key pairs generated before the timed ones")
ap.add_argument("--check", action="store_true", help="compare the keys with the other leg's for the same seed")
args = ap.parse_args()

import numpy as np
from eva import save
from eva.ckks import CKKSParameters
from eva.seal import generate_keys
from eva_amd import workloads

device = bool(args.device)
if args.what == "harris":
    compiled, params, sig, inputs = workloads.compile_config("c3")
else:
    compiled, params = None, CKKSParameters([60] + [50] * 9 + [60], set(), 1 << 16)


sampling = args.sampling == "device"


def keygen(on_device):
    if sampling:
        return generate_keys(params, 1, device_keygen=on_device, device_sampling=True)
    return generate_keys(params, 1, device_keygen=True) if on_device else generate_keys(params, 1, compress_keys=True)


t = []
for i in range(args.warmup + max(1, args.repeat)):
    pub = sec = None   # one key pair's device state at a time
    t0 = time.perf_counter()
    pub, sec = keygen(device)
    if i >= args.warmup:
        t.append(time.perf_counter() - t0)
t.sort()
assert pub.keys_compressed
st = pub.transfer_stats()
N, k = pub.poly_modulus_degree, len(pub.primes)
n_keys = len(pub.key_seeds())
line = (f"{args.what} device_keygen={int(device)} device_sampling={int(sampling)}: N={N} k={k} keys={n_keys} "
        f"generate_keys median {t[len(t) // 2]:.3f} s, "
        f"min {t[0]:.3f} s over {len(t)}; during keygen {st['h2d_bytes']} bytes h2d, {st['d2h_bytes']} bytes d2h; "
        f"key bytes held on the host {pub.key_host_bytes()}; key bytes in HBM after keygen {pub.key_bytes()[-1]}")
if args.check:
    other, _ = keygen(not device)
    a, b = pub.key_seeds(), other.key_seeds()
    same = sorted(a) == sorted(b) and all(np.array_equal(a[e], b[e]) for e in a) and np.array_equal(pub.relin_key(), other.relin_key())
    ga, gb = pub.galois_keys(), other.galois_keys()
    same = same and all(np.array_equal(ga[e], gb[e]) for e in ga)
    line += f"; same keys as the other leg: {same}"
    del other, ga, gb
if compiled is not None:
    enc = pub.encrypt(inputs, sig)
    pub.synchronize()
    t0 = time.perf_counter()
    pub.execute(compiled, enc)
    pub.synchronize()
    dt = time.perf_counter() - t0
    line += f"; first execute() {dt * 1e3:.2f} ms, key bytes in HBM after it {pub.key_bytes()[-1]}"
with tempfile.TemporaryDirectory() as tmp:
    d2h = pub.transfer_stats()["d2h_bytes"]
    t0 = time.perf_counter()
    save(pub, os.path.join(tmp, "ctx.sealpub"))
    dt = time.perf_counter() - t0
    line += f"; first save() {dt * 1e3:.2f} ms, {pub.transfer_stats()['d2h_bytes'] - d2h} bytes d2h during it"
print(line)
