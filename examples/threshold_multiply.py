#!/usr/bin/env python
"""Multiplying ciphertexts under a key nobody holds.

    PYTHONPATH=. python examples/threshold_multiply.py

Three parties generate their keys from one common seed.  Their public keys and Galois keys add up to the collective ones
(DESIGN.md 1.14); the relinearization key does not — s^2 is not the sum of the s_p^2 — so they run two rounds for it:

    round 1   every party:  eph, share1 = secret.relin_round1()        share1 is public, eph stays with the party
    anyone:                 agg1 = combine_relin_shares(all share1)
    round 2   every party:  share2 = secret.relin_round2(eph, agg1)    eph serves once and is wiped
    anyone:                 combine_public_contexts(publics, relin_round1=agg1, relin_round2=all share2)

The collective context then runs any compiled program — here the README polynomial 3 x^2 + 5 x - 2 — and the result is
opened only when every party contributes a decryption share.  The parties are semi-honest and all of them are needed
(P-of-P); a party that leaks its eph leaks its secret key."""
import os

import numpy as np

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import combine_public_contexts, combine_relin_shares, generate_keys

VEC, SMUDGE = 64, 40


def main():
    poly = EvaProgram("Polynomial", vec_size=VEC)
    with poly:
        x = Input("x")
        Output("y", 3 * x ** 2 + 5 * x - 2)
    poly.set_input_scales(50)   # the result leaves at scale 2^90: a 40-bit flood costs N * 3 * 2^40 / 2^90 per slot
    poly.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={"warn_vec_size": "false"}).compile(poly)

    common_seed = os.urandom(32)   # public: agreed on by the parties, e.g. a hash of their commitments
    parties = [generate_keys(params, common_seed=common_seed) for _ in range(3)]

    round1 = [secret.relin_round1() for _, secret in parties]            # each on its own party's machine
    agg1 = combine_relin_shares([share for _, share in round1])          # anywhere: public words only
    round2 = [secret.relin_round2(eph, agg1) for (_, secret), (eph, _) in zip(parties, round1)]
    collective = combine_public_contexts([public for public, _ in parties], relin_round1=agg1, relin_round2=round2)
    print(f"collective context: has_relin_key = {collective.has_relin_key}, key of {agg1.n_digits} digits, "
          f"N = {collective.poly_modulus_degree}, {len(collective.primes)} primes")

    xs = np.random.default_rng(0).uniform(-1, 1, VEC)
    out = collective.execute(compiled, collective.encrypt({"x": xs.tolist()}, sig))
    scale = out.get("y")[3]
    shares = [secret.decrypt_share(out, SMUDGE) for _, secret in parties]
    got = np.array(collective.combine_shares(out, shares, sig)["y"])
    want = 3 * xs ** 2 + 5 * xs - 2
    print(f"3 x^2 + 5 x - 2 under the collective key, opened by 3 shares: max error {np.abs(got - want).max():.3e} "
          f"(of which the flood accounts for at most {collective.poly_modulus_degree * 3 * 2.0 ** SMUDGE / scale:.3e})")
    alone = np.array(parties[0][1].decrypt(out, sig)["y"])
    print(f"  party 0 alone decrypts noise: max error {np.abs(alone - want).max():.3e}")
    try:
        parties[0][1].relin_round2(round1[0][0], agg1)
    except ValueError as e:
        print("  a second round 2 with the same ephemeral state is refused:", e)


if __name__ == "__main__":
    main()
