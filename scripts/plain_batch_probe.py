"""Per-instance unencrypted inputs in execute_batch: 256 Sobel-shaped instances at N = 2^14 whose image is
multiplied by an unencrypted gain vector before the filter.
  rows    execute_batch with a gain that differs per instance (one batched plaintext per group)
  shared  execute_batch with one gain for all instances (the path that existed before)
  loop    one execute() per instance: the only way to run differing gains without per-instance plaintexts
Median of --reps timed runs after --warmup untimed ones; one JSON line per mode.  A build without per-instance plaintexts
refuses `rows` ("must be the same for every instance"): the line then says so instead of a figure.
  python scripts/plain_batch_probe.py [--modes rows,shared,loop] [--batch 256] [--logn 14]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=ROOT, help="tree whose eva_amd package is measured")
ap.add_argument("--modes", default="rows,shared,loop")
ap.add_argument("--batch", type=int, default=256)
ap.add_argument("--logn", type=int, default=14)
ap.add_argument("--chunk", type=int, default=32)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
args = ap.parse_args()
sys.path.insert(0, args.root)

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys
from eva_amd.workloads import SOBEL_FILTER, _convolution_xy

VEC, W = 4096, 64
prog = EvaProgram('sobel_gain', vec_size=VEC)
with prog:
    img = Input('image') * Input('gain', False)
    a1, a2, a3 = 2.2137874823876622, -1.0984324107372518, 0.17254603006834726
    ch, cv = _convolution_xy(img, W, SOBEL_FILTER)
    x = ch ** 2 + cv ** 2
    Output('image', x * a1 + x ** 2 * a2 + x ** 3 * a3)
prog.set_input_scales(25)
prog.set_output_ranges(10)
compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
params.poly_modulus_degree = 1 << args.logn
pub, sec = generate_keys(params, 1)
pub.batch_chunk = args.chunk

B = args.batch
image = lambda u: [((37 * i + u) % 256) / 255.0 for i in range(VEC)]
gain = lambda u: [0.5 + ((i + 3 * u) % 7) / 16.0 for i in range(VEC)]
rows = [{'image': image(u), 'gain': gain(u)} for u in range(B)]
same = [{'image': image(u), 'gain': gain(0)} for u in range(B)]
enc_rows = pub.encrypt_batch(rows, sig, device_sampling=True)
enc_same = pub.encrypt_batch(same, sig, device_sampling=True)


def run(mode):
    if mode == "rows":
        pub.execute_batch(compiled, enc_rows)
    elif mode == "shared":
        pub.execute_batch(compiled, enc_same)
    else:
        for e in enc_rows:
            pub.execute(compiled, e)
        pub.synchronize()


for mode in args.modes.split(","):
    line = {"mode": mode, "workload": f"{B} Sobel instances with an unencrypted gain, N=2^{args.logn}, primes={list(params.prime_bits)}",
            "batch_chunk": args.chunk}
    try:
        for _ in range(args.warmup):
            run(mode)
        secs = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            run(mode)
            secs.append(time.perf_counter() - t0)
        med = statistics.median(secs)
        line.update({"median_ms": round(med * 1e3, 3), "dags_per_s": round(B / med, 1), "min_ms": round(min(secs) * 1e3, 3),
                     "max_ms": round(max(secs) * 1e3, 3)})
    except RuntimeError as e:
        line["refused"] = str(e)
    print(json.dumps(line), flush=True)
