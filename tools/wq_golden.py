#!/usr/bin/env python
"""Records tests/golden/wq_formats_parent.npz: what the four weight-only quantisers and their packers give, array for array, for one 8 x 128 and
one 6 x 192 bf16 matrix (N % 4 != 0: the packers pad).  tests/test_host_wq_formats.py holds weights.py to it bit for bit, so it is recorded
BEFORE a change to weights.py, never after.

    python tools/wq_golden.py tests/golden/wq_formats_parent.npz

Rows 0 and 1 of each matrix are built, block by block of 32 (values that are exact in bf16, a block scale of 2^0 unless said):
  row 0: an all-zero block; a block whose amax is the power of two 4; every rounding tie of the e2m1 grid, both signs, with -0.25 (a negative
         that rounds to zero) and amax 6; every rounding tie of the e2m3 grid with amax 7.5
  row 1: values above both saturation points (6.5 .. 7.875); the e2m3 ties negated, with -0.03125 and -0.0625 (negatives that round to zero);
         a block of amax 2^-124 (scale byte 1 before the clamp: 2); a block of amax 2^127 (scale byte 252, the upper clamp)
The other rows are normal draws at several magnitudes."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FORMATS = ("fp8", "nf4", "mxfp4", "mxfp6")
SHAPES = ((8, 128), (6, 192))


def matrix(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) * torch.tensor([2.0 ** (3 * i - 9) for i in range(n)])[:, None]
    blk = lambda vals: torch.tensor((list(vals) + [0.0] * 32)[:32])
    ties4 = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    ties6 = [i / 16 for i in range(1, 32, 2)] + [2 + i / 8 for i in range(1, 16, 2)] + [4 + i / 4 for i in range(1, 14, 2)]
    w[0, 0:32] = 0.0
    w[0, 32:64] = blk([4.0, -3.0, 1.0, 0.5, -0.75, 2.0, 0.125, -0.375] * 4)
    w[0, 64:96] = blk(ties4 + [-v for v in ties4] + [6.0, -0.25, -0.125, 0.125, 3.0, -6.0, 0.5, 1.0])
    w[0, 96:128] = blk(ties6 + [7.5])
    w[1, 0:32] = blk([6.5, 7.0, 7.75, 7.875, -6.5, -7.0, -7.75, -7.875, 6.25, 5.5, -5.5, 7.5, 7.25, -7.625] + [1.0] * 18)
    w[1, 32:64] = blk([-v for v in ties6] + [-7.5])
    w[1, 60], w[1, 61] = -0.03125, -0.0625            # in place of two ties; the block keeps amax 7.5
    w[1, 64:96] = torch.randn(32, generator=g).clamp(-1, 1) * 2.0 ** -124
    w[1, 64] = 2.0 ** -124
    w[1, 96:128] = torch.randn(32, generator=g).clamp(-1, 1) * 2.0 ** 127
    w[1, 96] = 2.0 ** 127
    return w.to(torch.bfloat16)


def outputs(W, fmt, w):
    """Every array the format's quantiser and packer give for the bf16 matrix w, by name"""
    n, k = w.shape
    if fmt == "fp8":
        return dict(zip(("codes", "scales", "eff"), W.quantize_e4m3_pow2(w)))
    quantise, pack, unpack = (getattr(W, f"{op}_{fmt}") for op in ("quantize", "pack", "unpack"))
    codes, scales, eff = quantise(w)
    packed, pscales = pack(codes, scales)
    ucodes, uscales = unpack(packed, pscales, n, k)
    return {"codes": codes, "scales": scales, "eff": eff, "packed": packed, "packed_scales": pscales, "unpacked_codes": ucodes, "unpacked_scales": uscales}


def main():
    from vibevoice_rocm_amd import weights as W
    out = {}
    for i, (n, k) in enumerate(SHAPES):
        w = matrix(n, k, 7 + i)
        out[f"w_{n}x{k}"] = w.float().numpy()
        for fmt in FORMATS:
            for name, t in outputs(W, fmt, w).items():
                out[f"{fmt}_{n}x{k}_{name}"] = t.numpy()
    np.savez_compressed(sys.argv[1], **out)
    print(f"{len(out)} arrays -> {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes)")


if __name__ == "__main__":
    main()
