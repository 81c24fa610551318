#!/usr/bin/env python
"""Opening a result that no single party can open.

    PYTHONPATH=. python examples/threshold_release.py

Three parties generate their keys from one common seed; the public halves add up to a collective public context whose
secret key s = s_0 + s_1 + s_2 nobody holds.  The server encrypts and computes under it (everything but relinearize here:
the relinearization key takes the two rounds of examples/threshold_multiply.py), and a result is opened only when every
party contributes a share:

    leg 1   program under the collective key  ->  decrypt_share x 3  ->  combine_shares
    leg 2   one owner's x^2 under the owner's key  ->  public_ctx.rekey to the collective key  ->  the same opening

smudge_bits is the parties' security parameter: a CKKS decryption leaks its noise, and the flood of 2^smudge_bits is what
hides it; it costs N * P * 2^smudge_bits / scale in every slot."""
import os

import numpy as np

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import combine_public_contexts, generate_keys

VEC, N, SMUDGE = 64, 4096, 40


def compile_program(name, build, scale_bits):
    prog = EvaProgram(name, vec_size=VEC)
    with prog:
        Output("y", build(Input("x")))
    prog.set_input_scales(scale_bits)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(prog)
    params.prime_bits = [60] * 4   # neither program rescales, so the chain is free
    params.poly_modulus_degree = N
    return compiled, params, sig


def open_jointly(collective, parties, enc, sig):
    shares = [secret.decrypt_share(enc, SMUDGE) for _, secret in parties]   # each on its own party's machine
    return np.array(collective.combine_shares(enc, shares, sig)["y"])       # anywhere: needs no secret key


def main():
    linear, params, sig = compile_program("linear", lambda x: (x << 1) * 0.5 + x, 30)
    common_seed = os.urandom(32)   # public: agreed on by the parties, e.g. a hash of their commitments
    parties = [generate_keys(params, common_seed=common_seed) for _ in range(3)]
    collective = combine_public_contexts([public for public, _ in parties])
    x = np.random.default_rng(0).uniform(-1, 1, VEC)

    out = collective.execute(linear, collective.encrypt({"x": x.tolist()}, sig))
    scale = out.get("y")[3]
    got = open_jointly(collective, parties, out, sig)
    want = np.roll(x, -1) * 0.5 + x
    print(f"leg 1, rotation and plaintext multiply under the collective key: max error {np.abs(got - want).max():.3e} "
          f"(the flood's bound {N * 3 * 2.0 ** SMUDGE / scale:.3e})")
    alone = np.array(parties[0][1].decrypt(out, sig)["y"])
    print(f"  party 0 alone decrypts noise: max error {np.abs(alone - want).max():.3e}")

    square, params2, sig2 = compile_program("square", lambda v: v * v, 50)
    owner_public, owner_secret = generate_keys(params2)
    rekey_key = owner_secret.make_rekey_key(collective)   # needs the collective PUBLIC key only
    result = owner_public.execute(square, owner_public.encrypt({"x": x.tolist()}, sig2))
    released = collective.rekey(result, rekey_key)
    got = open_jointly(collective, parties, released, sig2)
    print(f"leg 2, the owner's x^2 released to the committee: max error {np.abs(got - x * x).max():.3e}")
    print("transfer_stats of party 0:", parties[0][1].transfer_stats())


if __name__ == "__main__":
    main()
