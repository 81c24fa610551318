"""The client side of a batch: what encrypting all inputs and decrypting all outputs costs around
execute_batch, one ciphertext at a time and with the batched calls.

  python scripts/client_batch_probe.py c4 --batch 0|1
      BASELINE config 4's shape: 256 Sobel inputs, N = 2^14.
  python scripts/client_batch_probe.py c3 --batch 0|1
      BASELINE config 3's shape: 64 Harris inputs, N = 2^15.

--batch 0 is the baseline: a loop of public_ctx.encrypt / secret_ctx.decrypt, the only path before the batched calls, on
the same box.  --batch 1 is public_ctx.encrypt_batch / secret_ctx.decrypt_batch.  Both legs run the same execute_batch
between them.  Each run prints one line: the median wall time of the three phases over --repeat runs after --warmup
runs (the first run builds tables and plans).  --secret encrypts with the secret key (seeded ciphertexts) instead.
--sampling device (with --batch 1) draws the encryption randomness on the device from a 32-byte key per value
(DESIGN.md 1.7); --sampling host, the default, is the host sampler.
--arrays 1 runs the three phases through the array calls: encrypt_array on a uint8 array (c4: the pixels
0 .. 255 themselves) or a float32 array (c3), execute_batch on the SEALValuationBatch, decrypt_array; the line then also
reports the bytes that crossed PCIe in the last run's encrypt phase and the evah_ct_stack counters over its execute_batch.
--device-arrays 1 (with --arrays 1) is the same pipeline on device memory: the arrays are staged in HBM
first, outside the timed region — as torch tensors on the GPU where torch is importable (encrypt_array then orders itself
behind torch's current stream), else in a backend.DeviceBuffer — encrypt_array reads them in place and
decrypt_array(device=True) leaves the results in HBM; the line then also reports the bytes the decrypt phase brought
down.  --out-dtype picks the type decrypt_array writes (f64, f32, u8) on either array leg.

Kernel launches per call: run one leg under the profiler, which this script never starts itself and with no counters in
that run,

  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python scripts/client_batch_probe.py c4 --batch 1 --repeat 1 --warmup 0 --phase encrypt

and count the rows of the kernel trace (--phase encrypt | decrypt runs that phase's calls alone after the set-up, so the
difference between two instance counts, --instances, is the launches the extra instances cost: 0 for the batched calls
up to 64 instances).
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("what", choices=["c4", "c3"])
ap.add_argument("--batch", type=int, choices=[0, 1], default=1)
ap.add_argument("--instances", type=int, default=0, help="instances (default: 256 for c4, 64 for c3)")
ap.add_argument("--repeat", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--secret", action="store_true", help="secret-key encryption (seeded ciphertexts)")
ap.add_argument("--sampling", choices=["host", "device"], default="host",
                help="device: encrypt_batch(..., device_sampling=True), the randomness drawn on the device (needs --batch 1)")
ap.add_argument("--phase", choices=["all", "encrypt", "decrypt"], default="all",
                help="encrypt: no execute_batch and no decryption; decrypt: one untimed encryption and execute_batch, then decryptions alone")
ap.add_argument("--arrays", type=int, choices=[0, 1], default=0,
                help="1: encrypt_array / execute_batch on the batch / decrypt_array, uint8 input for c4 and float32 input for c3")
ap.add_argument("--device-arrays", type=int, choices=[0, 1], default=0,
                help="1 (with --arrays 1): the arrays staged in HBM before the timed region, decrypt_array(device=True)")
ap.add_argument("--out-dtype", choices=["f64", "f32", "u8"], default="f64", help="what decrypt_array writes on the array legs")
args = ap.parse_args()
if args.device_arrays and not args.arrays:
    ap.error("--device-arrays 1 needs --arrays 1")
if args.sampling == "device" and not args.batch:
    ap.error("--sampling device needs --batch 1: the single calls sample on the host")

import numpy as np

from eva.seal import generate_keys
from eva_amd import workloads

compiled, params, sig, _ = workloads.compile_config(args.what)
B = args.instances or {"c4": 256, "c3": 64}[args.what]
xs = [workloads.image(4096, shift=b) for b in range(B)]
pub, sec = generate_keys(params, 1)
batched = bool(args.batch)
enc_ctx = sec if args.secret else pub
on_device = args.sampling == "device"
arrays = None
if args.arrays:
    if args.what == "c4":   # the pixels as the camera gives them
        arrays = {'image': np.array([workloads.image(4096, shift=b, scale=1.0)['image'] for b in range(B)], dtype=np.uint8)}
    else:
        arrays = {'image': np.array([x['image'] for x in xs], dtype=np.float32)}
out_dtype = {"f64": np.float64, "f32": np.float32, "u8": np.uint8}[args.out_dtype]
staged = None
if args.device_arrays:
    try:
        import torch
        arrays = {n: torch.from_numpy(a).to("cuda") for n, a in arrays.items()}
        torch.cuda.synchronize()
        staged = "torch"
    except ImportError:
        from eva_amd import backend
        from eva_amd.hostref import coeff_modulus_create
        stage = backend.Context(1024, coeff_modulus_create(1024, [40, 40]))
        views = {}
        for n, a in arrays.items():
            buf = stage.buffer((a.nbytes + 7) // 8)
            buf.upload_bytes(a)
            views[n] = buf.view(a.shape, a.dtype)
        arrays = views
        staged = "DeviceBuffer"


def encrypt():
    if arrays:
        return enc_ctx.encrypt_array(arrays, sig)
    return enc_ctx.encrypt_batch(xs, sig, device_sampling=on_device) if batched else [enc_ctx.encrypt(x, sig) for x in xs]


def decrypt(outs):
    if arrays:
        return next(iter(sec.decrypt_array(outs, sig, dtype=out_dtype, device=bool(args.device_arrays)).values()))
    return sec.decrypt_batch(outs, sig) if batched else [sec.decrypt(o, sig) for o in outs]


t_enc, t_exe, t_dec = [], [], []
outs = None
h2d = d2h = stacked = None
if args.phase == "decrypt":
    outs = pub.execute_batch(compiled, encrypt())
    pub.synchronize()
for run in range(args.warmup + args.repeat):
    keep = run >= args.warmup
    if args.phase != "decrypt":
        pub.synchronize()
        before = pub.transfer_stats()
        t0 = time.perf_counter()
        encs = encrypt()
        pub.synchronize()
        t1 = time.perf_counter()
        h2d = pub.transfer_stats()["h2d_bytes"] - before["h2d_bytes"]
        if keep:
            t_enc.append(t1 - t0)
        if args.phase == "encrypt":
            continue
        s0 = pub.stack_stats()
        outs = pub.execute_batch(compiled, encs)
        pub.synchronize()
        t2 = time.perf_counter()
        s1 = pub.stack_stats()
        stacked = (s1["calls"] - s0["calls"], s1["instances"] - s0["instances"])
        if keep:
            t_exe.append(t2 - t1)
    d0 = pub.transfer_stats()["d2h_bytes"]
    t2 = time.perf_counter()
    got = decrypt(outs)
    t3 = time.perf_counter()
    d2h = pub.transfer_stats()["d2h_bytes"] - d0
    if keep:
        t_dec.append(t3 - t2)
    assert (got.shape[0] if args.device_arrays else len(got)) == B


def med(t):
    return f"{statistics.median(t) * 1e3:.2f} ms ({min(t) * 1e3:.2f} .. {max(t) * 1e3:.2f})" if t else "-"


extra = ""
if h2d is not None:
    extra += f", encrypt h2d {h2d} bytes"
if args.arrays and d2h is not None:
    extra += f", decrypt d2h {d2h} bytes (counted for uint8 and device rows only), out {args.out_dtype}"
if staged:
    extra += f", arrays staged as {staged}"
if stacked is not None:
    extra += f", evah_ct_stack over execute_batch {stacked[0]} calls / {stacked[1]} instances"
print(f"{args.what} batch={int(batched)} secret={int(args.secret)} sampling={args.sampling} arrays={args.arrays} device_arrays={args.device_arrays}: N={pub.poly_modulus_degree} k={len(pub.primes)} instances={B}; "
      f"medians over {args.repeat} runs after {args.warmup} warm-up: encrypt all inputs {med(t_enc)}, execute_batch {med(t_exe)}, "
      f"decrypt all outputs {med(t_dec)}{extra}")
