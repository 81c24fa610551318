#!/usr/bin/env python
"""Two encrypted programs under two key pairs on one GPU, chained through device memory.

    PYTHONPATH=. python examples/device_pipeline.py [--batch 70]

Stage A blurs a batch of 8x8 uint8 images under key pair A (N = 4096); its result is decrypted INTO device memory
(decrypt_array(device=True), uint8 out) and encrypted from there under key pair B (N = 2048), which runs stage B, a
horizontal gradient.  Decrypting under A and re-encrypting under B is the only way to chain EVA programs whose parameters
differ; with device arrays no pixel crosses PCIe in between, which transfer_stats() shows: pair B's context receives 64
bytes of randomness per image and sends back the 8-byte encodability sum of each row, and pair A's moves nothing.
The images start on the GPU as well: as a torch tensor where torch is importable, else in a backend.DeviceBuffer."""
import argparse

import numpy as np

from eva import EvaProgram, Input, Output
from eva.ckks import CKKSCompiler
from eva.seal import generate_keys

SIDE = 8
VEC = SIDE * SIDE


def compile_stage(name, build, N):
    prog = EvaProgram(name, vec_size=VEC)
    with prog:
        Output('image', build(Input('image')))
    prog.set_input_scales(30)
    prog.set_output_ranges(20)
    compiled, params, sig = CKKSCompiler(config={'warn_vec_size': 'false'}).compile(prog)
    params.poly_modulus_degree = N
    return compiled, params, sig


def blur(image):   # mean of a pixel and its right and lower neighbours (row-major rotations)
    return (image + (image << 1) + (image << SIDE)) * (1.0 / 3.0)


def gradient(image):
    return (image << 1) - image


def on_device(pixels):
    """the images in HBM before any encrypted work: a torch tensor, or rows in a DeviceBuffer"""
    try:
        import torch
        return torch.from_numpy(pixels).to("cuda"), "torch tensor"
    except ImportError:
        from eva_amd import backend
        from eva_amd.hostref import coeff_modulus_create
        stage = backend.Context(1024, coeff_modulus_create(1024, [40, 40]))
        buf = stage.buffer((pixels.nbytes + 7) // 8)
        buf.upload_bytes(pixels)
        return buf.view(pixels.shape, pixels.dtype), "DeviceBuffer"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=70)
    args = ap.parse_args()
    B = args.batch
    prog_a, params_a, sig_a = compile_stage('blur', blur, 4096)
    prog_b, params_b, sig_b = compile_stage('gradient', gradient, 2048)
    pub_a, sec_a = generate_keys(params_a)
    pub_b, sec_b = generate_keys(params_b)
    pixels = np.random.default_rng(1).integers(0, 256, size=(B, VEC), dtype=np.uint8)
    images, kind = on_device(pixels)

    enc_a = sec_a.encrypt_array({'image': images}, sig_a)           # read in place: no pixel crosses PCIe
    out_a = pub_a.execute_batch(prog_a, enc_a)
    a0 = pub_a.transfer_stats()
    blurred = sec_a.decrypt_array(out_a, sig_a, dtype=np.uint8, device=True)['image']   # [B, 64] uint8 in HBM
    for half in (pub_b, sec_b):                                     # (pair B's keys and tables go up here, once, and its public
        half.encrypt_array({'image': blurred}, sig_b)               #  half joins the device state whose counters it reports)
    b0 = pub_b.transfer_stats()
    enc_b = sec_b.encrypt_array({'image': blurred}, sig_b)          # pair A's output is pair B's input, where it lies
    a1, b1 = pub_a.transfer_stats(), pub_b.transfer_stats()
    out_b = pub_b.execute_batch(prog_b, enc_b)
    result = sec_b.decrypt_array(out_b, sig_b, dtype=np.float32)['image']

    clear_blur = np.clip(np.rint((pixels.astype(np.float64) + np.roll(pixels, -1, axis=1) + np.roll(pixels, -SIDE, axis=1)) / 3.0), 0, 255)
    mid = blurred.to_numpy()
    off = np.abs(mid.astype(np.float64) - clear_blur).max()
    clear = np.roll(mid.astype(np.float64), -1, axis=1) - mid
    print(f"{B} images of {SIDE}x{SIDE} uint8 pixels, staged as a {kind}")
    print(f"stage A (blur, N=4096) -> uint8 in device memory: largest difference from the clear blur {off:.0f} (a tie may round either way)")
    print(f"stage B (gradient, N=2048): largest error against the clear computation on stage A's pixels {np.abs(result - clear).max():.2e}")
    print(f"between the stages, pair A's context: h2d {a1['h2d_bytes'] - a0['h2d_bytes']} bytes, d2h {a1['d2h_bytes'] - a0['d2h_bytes']} bytes")
    print(f"                    pair B's context: h2d {b1['h2d_bytes'] - b0['h2d_bytes']} bytes (64 per image: an error key and a seed), "
          f"d2h {b1['d2h_bytes'] - b0['d2h_bytes']} bytes (8 per image: its row sum); value bytes: 0")
    assert a1['h2d_bytes'] == a0['h2d_bytes'] and a1['d2h_bytes'] == a0['d2h_bytes']
    assert b1['h2d_bytes'] - b0['h2d_bytes'] == 64 * B and b1['d2h_bytes'] - b0['d2h_bytes'] == 8 * B
    assert off <= 1 and np.abs(result - clear).max() < 1e-2


if __name__ == "__main__":
    main()
