#!/usr/bin/env python
"""A computation deeper than its modulus chain: one compiled program, run four times under one key pair.

    PYTHONPATH=. python examples/iterated_refresh.py [--passes 4]

The program is one step x <- x*x*0.5 + 0.25*x, compiled once; its chain has exactly the primes one step needs.  Between
the steps the key holder refreshes the result: secret_ctx.refresh decrypts it, divides the integer message by the power
of two between the result's scale and the input's, and encrypts it again at the top of the chain — exact integer
arithmetic on the GPU, no decode, no encode.  transfer_stats() shows what crosses PCIe for it: 64 bytes of randomness up
per value, nothing down.  Without a GPU (or with EVA_DEVICE_CLIENT=0) the refresh takes its host twin and gives the same
words; execute() itself needs the MI355X."""
import argparse

import numpy as np

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys

VEC = 64


def step(x):
    return x * x * 0.5 + 0.25 * x


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--passes", type=int, default=4)
    args = ap.parse_args()

    prog = EvaProgram("step", vec_size=VEC)
    with prog:
        Output("y", step(Input("x")))
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.poly_modulus_degree = 4096
    print(f"chain {list(params.prime_bits)} at N = 4096: one step deep; running {args.passes}")

    public_ctx, secret_ctx = generate_keys(params)
    x = np.random.default_rng(0).uniform(-1, 1, VEC)
    enc, want = secret_ctx.encrypt({"x": x.tolist()}, sig), x
    for p in range(args.passes):
        out = public_ctx.execute(compiled, enc)
        want = step(want)
        got = np.array(secret_ctx.decrypt(out, sig)["y"])
        print(f"pass {p + 1}: max error against numpy {np.abs(got - want).max():.3e}")
        if p + 1 < args.passes:
            before = public_ctx.transfer_stats()
            enc = secret_ctx.refresh(out, sig, rename={"x": "y"})   # the result "y" becomes the next pass's input "x"
            after = public_ctx.transfer_stats()
            print(f"  refresh: {after['h2d_bytes'] - before['h2d_bytes']} bytes up, {after['d2h_bytes'] - before['d2h_bytes']} bytes down")


if __name__ == "__main__":
    main()
