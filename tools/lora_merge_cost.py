"""What the load-time LoRA merge costs: the merge kernel alone at Llama-3-8B's matrix shapes.

    python tools/lora_merge_cost.py [--iters 20] [--out profiles/lora_merge.txt]

mx_lora_merge_probe launches the production kernel (csrc/lora.hip) on random data: one launch whose result is
copied back, two warm-up launches, then `iters` launches between two HIP events on one stream; the mean is the time
per launch.  The kernel reads and writes the bf16 matrix once, 2 * rows * cols * 2 bytes, and that traffic over the
time is its rate.  The yardstick is mx_probe_copy in the same process over the same number of bytes per buffer: a
device-to-device copy moves the same traffic (read + written) with no arithmetic and no second operand.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(4096, 4096, "attn_q / attn_output"), (14336, 4096, "ffn_gate / ffn_up"), (4096, 14336, "ffn_down")]
RANKS = (16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.iters < 20:
        raise SystemExit("--iters must be at least 20")
    from llama_p2p_amd import engine as E

    lib = E.lib()
    rng = np.random.default_rng(0)
    lines = [f"LoRA merge kernel (lora_merge_kernel, csrc/lora.hip) through mx_lora_merge_probe: mean of {a.iters} "
             f"launches between two HIP events after 1 + 2 warm-up launches; traffic = 2 * rows * cols * 2 B (the bf16 "
             f"matrix read and written once); copy = mx_probe_copy (read + written bytes / s, best variant, {a.iters} "
             f"passes) over buffers of rows * cols * 2 B in the same process"]
    for rows, cols, what in SHAPES:
        nbytes = rows * cols * 2
        gbs = ctypes.c_double()
        desc = ctypes.create_string_buffer(160)
        rc = lib.mx_probe_copy(a.device, nbytes, a.iters, ctypes.byref(gbs), desc, len(desc))
        if rc != E.MX_OK:
            raise SystemExit(f"mx_probe_copy: {lib.mx_last_error().decode()}")
        w = rng.integers(0x3C00, 0x3D00, (rows, cols)).astype(np.uint16)  # bf16 values around 0.01 .. 0.03
        for r in RANKS:
            A = (0.02 * rng.standard_normal((r, cols))).astype(np.float32)
            B = (0.02 * rng.standard_normal((rows, r))).astype(np.float32)
            _, guard, us = E.lora_merge_probe(w, A, B, 2.0 ** -10, iters=a.iters, device=a.device)
            if not (guard == 0xFFFF).all():
                raise SystemExit("guard overwritten")
            rate = 2 * nbytes / (us * 1e-6) / 1e9
            lines.append(f"{rows} x {cols} ({what}), r = {r}: {us:.1f} us per launch, {rate:.0f} GB/s; copy of the same "
                         f"bytes: {gbs.value:.0f} GB/s ({desc.value.decode()}); merge / copy = {rate / gbs.value:.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
