"""Weight-only OCP MXFP4 (weight_quant="mxfp4"), host side, no GPU: the quantiser against hand-written cases of the MX v1.0 conversion, the
VV_MXFP4 packers, and the wiring through weights.py, _lib.py and the header."""
import os
import re

import pytest
import torch

from vibevoice_rocm_amd import _lib
from vibevoice_rocm_amd.weights import (MXFP4_VALUES, fp8_matrix_names, mxfp4_effective_state_dict, pack_mxfp4, quantize_mxfp4, unpack_mxfp4)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(vals, fill=0.0):
    """one row of one 32-block: vals, then `fill`"""
    return torch.tensor([list(vals) + [fill] * (32 - len(vals))], dtype=torch.float32)


def test_code_table_is_the_formats():
    """codes 0..7 are +0, 0.5, 1, 1.5, 2, 3, 4, 6 and 8..15 the same negated: each value, in a block whose scale is 2^0, takes its own code"""
    assert MXFP4_VALUES == (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
    vals = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    codes, e, eff = quantize_mxfp4(_block(vals + [-v for v in vals]))
    assert e.tolist() == [[127]], "max |w| = 6: floor(log2 6) - 2 = 0"
    assert codes[0, :16].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 12, 13, 14, 15], "a value that is zero takes code 0, never code 8"
    assert eff[0, :16].tolist() == vals + [-v for v in vals]
    assert codes.dtype == e.dtype == torch.uint8 and eff.dtype == torch.float32


def test_ties_round_to_even_and_large_values_saturate():
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0]
    x = _block(ties + [-t for t in ties] + [7.9])         # 7.9 holds the block's scale at 2^0: floor(log2 7.9) = 2
    codes, e, eff = quantize_mxfp4(x)
    assert e.tolist() == [[127]]
    assert eff[0, :7].tolist() == want and eff[0, 7:14].tolist() == [-w for w in want]
    assert codes[0, :7].tolist() == [0, 2, 2, 4, 4, 6, 6] and codes[0, 7:14].tolist() == [0, 10, 10, 12, 12, 14, 14]
    # just off the ties, to either side
    near = [0.2499, 0.2501, 1.2499, 1.2501, 2.4999, 2.5001, 4.9999, 5.0001]
    assert quantize_mxfp4(_block(near + [7.9]))[2][0, :8].tolist() == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    # anything above 6 saturates: 6.0001 .. 7.9999 with the scale at 2^0
    sat = [6.0001, 6.5, 7.0, 7.5, 7.9999]
    codes, e, eff = quantize_mxfp4(_block(sat + [-s for s in sat]))
    assert e.tolist() == [[127]] and codes[0, :10].tolist() == [7] * 5 + [15] * 5 and eff[0, :10].tolist() == [6.0] * 5 + [-6.0] * 5


def test_scale_byte_rule_and_clamps():
    """scale byte = clamp(floor(log2 max|w|) - 2 + 127, 2, 252) on blocks with max |w| from 2^-20 to 2^10, at the power of two, just below
    the next one and in between; the clamps; the all-zero block"""
    for p in range(-20, 11):
        for frac in (1.0, 1.5, 1.9999999):
            amax = frac * 2.0 ** p
            x = _block([amax, -0.3 * amax, 0.01 * amax])
            codes, e, eff = quantize_mxfp4(x)
            assert e.tolist() == [[p - 2 + 127]], (p, frac, e)
            s = 2.0 ** (p - 2)
            assert eff[0, 0].item() == {1.0: 4.0, 1.5: 6.0, 1.9999999: 6.0}[frac] * s       # 4 s, 6 s, and 7.99.. s saturating at 6 s
    tiny = _block([2.0 ** -140, 2.0 ** -126, -(2.0 ** -125)])
    codes, e, eff = quantize_mxfp4(tiny)
    assert e.tolist() == [[2]], "floor(log2) - 2 + 127 = 0 here: clamped to 2"
    assert codes[0, :3].tolist() == [0, 1, 10] and eff[0, :3].tolist() == [0.0, 2.0 ** -126, -(2.0 ** -125)]
    huge = _block([3.0e38, -1.0e38])
    codes, e, eff = quantize_mxfp4(huge)
    assert e.tolist() == [[252]] and codes[0, :2].tolist() == [7, 12]                        # 3e38 / 2^125 = 7.05 -> 6; -1e38 / 2^125 = -2.35 -> -2
    assert eff[0, 0].item() == 6 * 2.0 ** 125 and torch.isfinite(eff).all()
    zero = torch.zeros(2, 64)
    zero[1, 40] = 1.0
    codes, e, eff = quantize_mxfp4(zero)
    assert e.tolist() == [[127, 127], [127, 125]] and int(codes.sum()) == 6 and bool((eff == zero).all())
    assert not torch.signbit(eff).any()
    with pytest.raises(ValueError, match="32"):
        quantize_mxfp4(torch.zeros(4, 48))


def test_effective_matrix_is_a_fixed_point_exact_in_bf16_and_within_one_scale():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(37, 544, generator=g) * torch.exp2(torch.randint(-12, 6, (37, 1), generator=g).float())
    w[3, 64:96] = 0.0
    codes, e, eff = quantize_mxfp4(w)
    c2, e2, eff2 = quantize_mxfp4(eff)
    assert torch.equal(codes, c2) and torch.equal(e, e2) and torch.equal(eff, eff2), "re-quantising the effective matrix changes nothing"
    assert torch.equal(eff.bfloat16().float(), eff), "value(code) * 2^(e - 127) is exact in bf16"
    scale = torch.exp2(e.float() - 127).repeat_interleave(32, dim=1)
    unsat = w.abs() <= 6 * scale
    assert bool(((w - eff).abs() <= scale)[unsat].all()), "an unsaturated element is within one scale (half the widest grid step) of its weight"
    assert float(unsat.float().mean()) > 0.9
    val = torch.tensor(MXFP4_VALUES + tuple(-v for v in MXFP4_VALUES))
    assert torch.equal(val[codes.long()] * scale, eff), "the effective weight is value(code) * 2^(e - 127)"
    assert int(e.min()) >= 2 and int(e.max()) <= 252


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("k", [32, 544, 1024])
def test_pack_unpack_round_trip_and_padding(n, k):
    g = torch.Generator().manual_seed(n * 1000 + k)
    codes = torch.randint(0, 16, (n, k), generator=g).to(torch.uint8)
    scales = torch.randint(2, 253, (n, k // 32), generator=g).to(torch.uint8)
    packed, sb = pack_mxfp4(codes, scales)
    nq, ku = (n + 3) // 4, (k + 511) // 512
    assert packed.dtype == sb.dtype == torch.uint8 and packed.numel() == nq * ku * 1024 and sb.numel() == nq * ku * 64
    c2, s2 = unpack_mxfp4(packed, sb, n, k)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    # the layout, element by element, as include/vv_hip.h words it
    dw = packed.view(-1, 4).int()
    dw = dw[:, 0] | (dw[:, 1] << 8) | (dw[:, 2] << 16) | (dw[:, 3] << 24)
    for row, col in ((0, 0), (n - 1, k - 1), (n // 2, k // 2 + 3), (n - 1, 17 % k)):
        q, r, u, l, i = row // 4, row % 4, col // 512, (col % 512) // 8, col % 8
        assert (int(dw[((q * ku + u) * 64 + l) * 4 + r]) >> (4 * i)) & 15 == int(codes[row, col])
        assert int(sb[((q * ku + u) * 16 + (col % 512) // 32) * 4 + r]) == int(scales[row, col // 32])
    # padding: rows past N and k past K hold code 0 and scale byte 127
    cf, sf = unpack_mxfp4(packed, sb, nq * 4, ku * 512)
    assert int(cf[n:].sum()) == 0 and int(cf[:, k:].sum()) == 0
    assert bool((sf[n:] == 127).all()) and bool((sf[:, k // 32:] == 127).all())


def test_weights_layer_accepts_mxfp4_and_still_refuses_unknown_modes():
    """DeviceWeights checks the mode before it touches a device: an unknown string raises the ValueError that names the built modes - 'mxfp4'
    among them - and mxfp4 with fp32 matrices raises the bf16 rule, which only an accepted mode reaches"""
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.weights import DeviceWeights
    cfg = VVConfig.preset("tiny")
    with pytest.raises(ValueError, match="mxfp4"):
        DeviceWeights(cfg, {}, "cpu", torch.bfloat16, quant="mxfp8")
    with pytest.raises(ValueError, match="torch_dtype must be bfloat16"):
        DeviceWeights(cfg, {}, "cpu", torch.float32, quant="mxfp4")
    with pytest.raises(ValueError, match="pre-quantized"):
        DeviceWeights(cfg, {}, "cpu", torch.bfloat16, quant="mxfp4", prequant={"x": object()})


def test_effective_state_dict_covers_k_multiples_of_32_only():
    from vibevoice_rocm_amd.config import VVConfig
    cfg = VVConfig.preset("tiny")
    names = fp8_matrix_names(cfg)
    g = torch.Generator().manual_seed(3)
    sd = {name: torch.randn(8, 64 if i % 2 else 48, generator=g).bfloat16() for i, name in enumerate(names)}
    sd["other.weight"] = torch.randn(8, 64, generator=g)
    out = mxfp4_effective_state_dict(cfg, sd)
    assert set(out) == set(sd) and out["other.weight"] is sd["other.weight"]
    for i, name in enumerate(names):
        if i % 2:
            assert out[name].dtype == torch.float32 and torch.equal(out[name], quantize_mxfp4(sd[name])[2]) and not torch.equal(out[name], sd[name].float())
        else:
            assert out[name] is sd[name], "K % 32 != 0: no companion, the matrix stays as it is"


def test_header_lib_and_docs_agree():
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    assert re.search(r"enum \{ VV_MXFP4 = 4 \};", hdr) and re.search(r"enum \{ VV_WQ_MXFP4 = 0x200 \};", hdr)
    assert (_lib.VV_MXFP4, _lib.VV_WQ_MXFP4, _lib.VV_NF4, _lib.VV_WQ_NF4) == (4, 0x200, 3, 0x100)
    assert "read as uint8_t" in hdr and "[ceil(N/4)][ceil(K/512)][16 blocks][4 rows]" in hdr
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(vv_[a-z0-9_]+)\s*\(", plain))
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    lib = _lib.load()
    assert lib.vv_abi_version() == 6
    assert "VV_MXFP4" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
