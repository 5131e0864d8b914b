"""CPU only: the four weight-only quantisers and their packers against tests/golden/wq_formats_parent.npz, recorded (tools/wq_golden.py) before
quantize_mxfp4 / quantize_mxfp6 became one function and the NF4 / MXFP4 packers one nibble interleave: every array bit for bit.  The two
matrices carry an all-zero block, a power-of-two amax, every rounding tie of the e2m1 and e2m3 grids, values beyond both saturation points,
negatives that round to zero and a block at each scale-byte clamp (2 and 252); 6 x 192 makes the packers pad (N % 4 != 0)."""
import os
import sys

import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import wq_golden  # noqa: E402

from vibevoice_rocm_amd import weights as W  # noqa: E402

GOLD = load_golden("wq_formats_parent")
CASES = [(fmt, n, k) for fmt in wq_golden.FORMATS for n, k in wq_golden.SHAPES]


def _input(n, k):
    return torch.from_numpy(GOLD[f"w_{n}x{k}"]).to(torch.bfloat16)


def test_the_inputs_hold_what_they_are_recorded_for():
    """the golden's own premise, read back from its arrays: both scale-byte clamps, the all-zero block's byte 127, every e2m1 / e2m3 code, and
    zero codes for the negatives that round to zero"""
    for n, k in wq_golden.SHAPES:
        assert torch.equal(_input(n, k).float(), torch.from_numpy(GOLD[f"w_{n}x{k}"])), "the recorded input is exact in bf16"
        for fmt, n_codes in (("mxfp4", 16), ("mxfp6", 64)):
            sc, codes = GOLD[f"{fmt}_{n}x{k}_scales"], GOLD[f"{fmt}_{n}x{k}_codes"]
            assert sc[0, 0] == 127 and not codes[0, :32].any()
            assert sc[1, 2] == W.MXFP4_SCALE_MIN and sc[1, 3] == W.MXFP4_SCALE_MAX
            assert len(set(codes.ravel().tolist()) | {n_codes // 2}) == n_codes, "every code but the negative zero occurs"
            assert n_codes // 2 not in codes
        assert not GOLD[f"mxfp6_{n}x{k}_codes"][1, 60:62].any() and GOLD[f"mxfp4_{n}x{k}_codes"][0, 64 + 15] == 0


@pytest.mark.parametrize("fmt,n,k", CASES, ids=[f"{f}-{n}x{k}" for f, n, k in CASES])
def test_quantisers_and_packers_are_bit_identical(fmt, n, k):
    got = wq_golden.outputs(W, fmt, _input(n, k))
    want = {name[len(f"{fmt}_{n}x{k}_"):]: torch.from_numpy(a) for name, a in GOLD.items() if name.startswith(f"{fmt}_{n}x{k}_")}
    assert set(got) == set(want) and len(want) == (3 if fmt == "fp8" else 7)
    for name, t in want.items():
        assert got[name].dtype == t.dtype and got[name].shape == t.shape, (name, got[name].dtype, got[name].shape)
        assert torch.equal(got[name], t), f"{fmt} {n}x{k}: {name} differs from the recorded array"
    if fmt != "fp8":      # unpack(pack(x)) == x
        assert torch.equal(got["unpacked_codes"], got["codes"]) and torch.equal(got["unpacked_scales"], got["scales"])


@pytest.mark.parametrize("quant", wq_golden.FORMATS)
def test_the_table_serves_the_old_names(quant):
    """effective_state_dict(cfg, sd, quant) is what <quant>_effective_state_dict gives, and the table's row is the format's own functions"""
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("tiny")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 5).items()}
    a, b = W.effective_state_dict(cfg, sd, quant), getattr(W, f"{quant}_effective_state_dict")(cfg, sd)
    assert a.keys() == b.keys() == sd.keys()
    changed = [k for k in sd if not torch.equal(a[k].float(), sd[k].float())]
    assert changed and set(changed) <= set(W.fp8_matrix_names(cfg))
    assert all(torch.equal(a[k], b[k]) and a[k].dtype == torch.float32 for k in changed)
    f = W.WEIGHT_FORMATS[quant]
    assert f.quantize is (W.quantize_e4m3_pow2 if quant == "fp8" else getattr(W, f"quantize_{quant}"))
    assert f.pack is (None if quant == "fp8" else getattr(W, f"pack_{quant}"))
    assert f.block == (None if quant == "fp8" else getattr(W, f"{quant.upper()}_BLOCK"))
