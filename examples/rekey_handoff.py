#!/usr/bin/env python
"""Handing a result to another key pair without a secret key in the room.

    PYTHONPATH=. python examples/rekey_handoff.py

Two key pairs A and B over the same parameters.  A makes a re-key key from B's PUBLIC context and gives it to the server;
from then on the server, which holds public contexts only, turns results under A into results under B:

    program under A  ->  public_ctx_B.rekey  ->  secret_ctx_B.decrypt
                                             ->  secret_ctx_B.refresh  ->  program under B

On one GPU no ciphertext byte crosses PCIe for it: B's context reads A's result where it lies.  B together with the
server learns A's secret key — that is inherent to proxy re-encryption; hand the key only to a server B does not collude
with, or use it for A's own replacement key after a key rotation."""
import numpy as np

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys

VEC = 64


def step(x):
    return x * x * 0.5 + 0.25 * x


def moved(ctx, before):
    after = ctx.transfer_stats()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def main():
    prog = EvaProgram("step", vec_size=VEC)
    with prog:
        Output("y", step(Input("x")))
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.poly_modulus_degree = 4096

    public_a, secret_a = generate_keys(params)
    public_b, secret_b = generate_keys(params)
    rekey_key = secret_a.make_rekey_key(public_b)   # A's side: needs A's secret key and B's public context
    print(f"re-key key A -> B: {rekey_key.n_digits} digits, {rekey_key.words().nbytes >> 10} KiB, sent whole")

    x = np.random.default_rng(0).uniform(-1, 1, VEC)
    out_a = public_a.execute(compiled, secret_a.encrypt({"x": x.tolist()}, sig))
    public_b.install_rekey_key(rekey_key)           # the server's side from here on: public contexts only
    public_a.synchronize()
    before_a, before_b = public_a.transfer_stats(), public_b.transfer_stats()
    out_b = public_b.rekey(out_a, rekey_key)
    print(f"rekey: moved across PCIe on A's state {moved(public_a, before_a)}, on B's {moved(public_b, before_b)}")

    got = np.array(secret_b.decrypt(out_b, sig)["y"])
    print(f"decrypted under B: max error against numpy {np.abs(got - step(x)).max():.3e}")
    ref = np.array(secret_a.decrypt(out_a, sig)["y"])
    print(f"  against A's own decryption of the same result {np.abs(got - ref).max():.3e}")

    enc_b = secret_b.refresh(out_b, sig, rename={"x": "y"})   # B brings it back to the top of the chain ...
    again = public_b.execute(compiled, enc_b)                 # ... and the next stage runs under B
    got = np.array(secret_b.decrypt(again, sig)["y"])
    print(f"second stage under B: max error against numpy {np.abs(got - step(step(x))).max():.3e}")
    print("transfer_stats A:", public_a.transfer_stats())
    print("transfer_stats B:", public_b.transfer_stats())


if __name__ == "__main__":
    main()
