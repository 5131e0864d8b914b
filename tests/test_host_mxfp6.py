"""Weight-only OCP MXFP6, the e2m3 element type (weight_quant="mxfp6"), host side, no GPU: the quantiser against hand-written cases of the MX
v1.0 conversion, the VV_MXFP6 packers, the fidelity the mode is built for (fp8's error at 0.78 of its bytes), and the wiring through
weights.py, modeling.py, _lib.py and the header."""
import os
import re

import pytest
import torch

from vibevoice_rocm_amd import _lib
from vibevoice_rocm_amd.weights import (MXFP6_VALUES, DeviceWeights, fp8_matrix_names, mxfp6_effective_state_dict, pack_mxfp6,
                                        quantize_e4m3_pow2, quantize_mxfp4, quantize_mxfp6, unpack_mxfp6)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _block(vals, fill=0.0):
    """one row of one 32-block: vals, then `fill`"""
    return torch.tensor([list(vals) + [fill] * (32 - len(vals))], dtype=torch.float32)


def test_code_table_is_the_formats():
    """code = E << 3 | m: E == 0 means m / 8, E in 1..3 means (1 + m / 8) * 2^(E - 1); codes 32..63 the same negated.  Each value, in a block
    whose scale is 2^0, takes its own code; a zero takes code 0, never code 32"""
    want = [m / 8 for m in range(8)] + [(1 + m / 8) * 2.0 ** (E - 1) for E in (1, 2, 3) for m in range(8)]
    assert list(MXFP6_VALUES) == want and want[-1] == 7.5 and want[8] == 1.0 and want[16] == 2.0 and want[24] == 4.0
    codes, e, eff = quantize_mxfp6(_block(want))
    assert e.tolist() == [[127]], "max |w| = 7.5: floor(log2 7.5) - 2 = 0"
    assert codes[0].tolist() == list(range(32)) and eff[0].tolist() == want
    codes, e, eff = quantize_mxfp6(_block([-v for v in want]))
    assert codes[0].tolist() == [0] + list(range(33, 64)) and eff[0].tolist() == [0.0] + [-v for v in want[1:]]
    assert not torch.signbit(eff[0, 0]), "the zero is +0"
    assert codes.dtype == e.dtype == torch.uint8 and eff.dtype == torch.float32


def test_largest_value_saturation_and_the_block_scale():
    """max |w| = 7.5 * 2^x is exact under scale 2^x; anything between 7.5 and 8 scales keeps the scale and saturates at 7.5 once it rounds past
    it (7.75 is the tie between 7.5 and the 8.0 the grid does not have: it saturates, as every value above it does)"""
    for x in (-9, 0, 3, 11):
        s = 2.0 ** x
        codes, e, eff = quantize_mxfp6(_block([7.5 * s, -7.5 * s, 0.125 * s]))
        assert e.tolist() == [[127 + x]] and codes[0, :3].tolist() == [31, 63, 1] and eff[0, :3].tolist() == [7.5 * s, -7.5 * s, 0.125 * s]
    sat = [7.5001, 7.74, 7.75, 7.76, 7.9999]
    codes, e, eff = quantize_mxfp6(_block(sat + [-v for v in sat]))
    assert e.tolist() == [[127]], "below 8 the scale stays 2^0"
    assert codes[0, :10].tolist() == [31] * 5 + [63] * 5 and eff[0, :10].tolist() == [7.5] * 5 + [-7.5] * 5
    codes, e, eff = quantize_mxfp6(_block([8.0, 7.9999]))
    assert e.tolist() == [[128]] and eff[0, :2].tolist() == [8.0, 8.0], "at 8 the scale doubles: 4.0 x 2, and 3.99995 rounds up to it"


def test_ties_round_to_even_on_each_spacing():
    """spacing 1/8 below 2 (subnormals and the first binade), 1/4 below 4, 1/2 up to 7.5: a tie goes to the even mantissa"""
    ties = [0.0625, 0.1875, 1.0625, 1.9375, 2.125, 2.375, 3.875, 4.25, 4.75, 7.25]
    want = [0.0, 0.25, 1.0, 2.0, 2.0, 2.5, 4.0, 4.0, 5.0, 7.0]
    x = _block(ties + [-t for t in ties] + [7.5])               # 7.5 holds the block's scale at 2^0
    codes, e, eff = quantize_mxfp6(x)
    assert e.tolist() == [[127]]
    assert eff[0, :10].tolist() == want and eff[0, 10:20].tolist() == [0.0] + [-w for w in want[1:]]
    assert codes[0, :10].tolist() == [0, 2, 8, 16, 16, 18, 24, 24, 26, 30]
    assert codes[0, 10:20].tolist() == [0, 34, 40, 48, 48, 50, 56, 56, 58, 62], "-0.0625 rounds to zero from below and takes code 0, not 32"
    assert not torch.signbit(eff[0, 10])
    near = [0.0624, 0.0626, 1.0624, 1.0626, 2.1249, 2.1251, 4.2499, 4.2501]            # just off the ties, to either side
    assert quantize_mxfp6(_block(near + [7.5]))[2][0, :8].tolist() == [0.0, 0.125, 1.0, 1.125, 2.0, 2.25, 4.0, 4.5]


def test_scale_byte_rule_and_clamps():
    """scale byte = clamp(floor(log2 max|w|) - 2 + 127, 2, 252) from 2^-20 to 2^10, at the power of two, in between and just below the next
    one; the clamp at 2 (scale 2^-125 for anything smaller), 252 at the top of fp32; the all-zero block gets 127"""
    for p in range(-20, 11):
        for frac in (1.0, 1.5, 1.9999999):
            amax = frac * 2.0 ** p
            codes, e, eff = quantize_mxfp6(_block([amax, -0.3 * amax, 0.01 * amax]))
            assert e.tolist() == [[p - 2 + 127]], (p, frac, e)
            assert eff[0, 0].item() == {1.0: 4.0, 1.5: 6.0, 1.9999999: 7.5}[frac] * 2.0 ** (p - 2)
    codes, e, eff = quantize_mxfp6(_block([2.0 ** -140, 2.0 ** -126, -(2.0 ** -125)]))
    assert e.tolist() == [[2]], "floor(log2) - 2 + 127 = 0 here: clamped to 2"
    assert codes[0, :3].tolist() == [0, 4, 40] and eff[0, :3].tolist() == [0.0, 2.0 ** -126, -(2.0 ** -125)]
    codes, e, eff = quantize_mxfp6(_block([3.0e38, -1.0e38]))
    assert e.tolist() == [[252]] and codes[0, :2].tolist() == [30, 49]          # 3e38 / 2^125 = 7.05 -> 7.0; -1e38 / 2^125 = -2.35 -> -2.25
    assert eff[0, 0].item() == 7 * 2.0 ** 125 and torch.isfinite(eff).all()
    zero = torch.zeros(2, 64)
    zero[1, 40] = 1.0
    codes, e, eff = quantize_mxfp6(zero)
    assert e.tolist() == [[127, 127], [127, 125]] and int(codes.sum()) == 24 and bool((eff == zero).all())      # 1.0 / 2^-2 = 4.0: code 24
    assert not torch.signbit(eff).any()
    with pytest.raises(ValueError, match="32"):
        quantize_mxfp6(torch.zeros(4, 48))


def test_effective_matrix_is_a_fixed_point_and_exact_in_bf16():
    g = torch.Generator().manual_seed(5)
    w = torch.randn(37, 544, generator=g) * torch.exp2(torch.randint(-12, 6, (37, 1), generator=g).float())
    w[3, 64:96] = 0.0
    codes, e, eff = quantize_mxfp6(w)
    c2, e2, eff2 = quantize_mxfp6(eff)
    assert torch.equal(codes, c2) and torch.equal(e, e2) and torch.equal(eff, eff2), "re-quantising the effective matrix changes nothing"
    assert torch.equal(eff.to(torch.bfloat16).float(), eff), "four significant bits times a power of two: exact in bf16"
    scale = torch.exp2(e.float() - 127).repeat_interleave(32, dim=1)
    unsat = w.abs() <= 7.5 * scale
    assert bool(((w - eff).abs() <= scale / 4)[unsat].all()), "an unsaturated element is within half the widest grid step of its weight"
    assert float(unsat.float().mean()) > 0.99
    val = torch.tensor(MXFP6_VALUES + tuple(-v for v in MXFP6_VALUES))
    assert torch.equal(val[codes.long()] * scale, eff), "the effective weight is value(code) * 2^(e - 127)"
    assert int(codes.max()) <= 63 and int(e.min()) >= 2 and int(e.max()) <= 252


def test_fidelity_is_fp8s_at_a_fraction_of_mxfp4s_error():
    """What the mode is for: on a Gaussian [512, 1536] matrix the effective matrix is at most 1.15 x as far (rel RMS) from the original as the
    fp8 mode's and at most 0.30 x as far as MXFP4's"""
    torch.manual_seed(0)
    w = torch.randn(512, 1536)

    def err(eff):
        return float(((eff - w) ** 2).mean().sqrt() / (w ** 2).mean().sqrt())
    f8, m6, m4 = err(quantize_e4m3_pow2(w)[2]), err(quantize_mxfp6(w)[2]), err(quantize_mxfp4(w)[2])
    print(f"rel RMS weight error: fp8 {f8:.4f}  mxfp6 {m6:.4f} ({m6 / f8:.3f} x fp8, {m6 / m4:.3f} x mxfp4)  mxfp4 {m4:.4f}")
    assert m6 <= 1.15 * f8, (m6, f8)
    assert m6 <= 0.30 * m4, (m6, m4)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("k", [32, 544, 2080])
def test_pack_unpack_round_trip_and_padding(n, k):
    g = torch.Generator().manual_seed(n * 10000 + k)
    codes = torch.randint(0, 64, (n, k), generator=g).to(torch.uint8)
    scales = torch.randint(2, 253, (n, k // 32), generator=g).to(torch.uint8)
    packed, sb = pack_mxfp6(codes, scales)
    nq, nb = (n + 3) // 4, k // 32
    assert packed.dtype == sb.dtype == torch.uint8 and packed.numel() == nq * 4 * nb * 24 and sb.numel() == nq * 4 * nb
    c2, s2 = unpack_mxfp6(packed, sb, n, k)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    # the layout, element by element, as include/vv_hip.h words it: bit j of code i is bit 6 i + j of the block's 192-bit string,
    # whose bytes 0..15 lie in plane A and 16..23 in plane B of the row group
    by = packed.tolist()
    for row, col in ((0, 0), (n - 1, k - 1), (n // 2, k // 2 + 3), (n - 1, 21 % k), (0, 31)):
        q, r, b, i = row // 4, row % 4, col // 32, col % 32
        got = 0
        for j in range(6):
            pos = 6 * i + j
            byte = pos // 8
            at = q * nb * 96 + ((r * nb + b) * 16 + byte if byte < 16 else nb * 64 + (r * nb + b) * 8 + byte - 16)
            got |= ((by[at] >> (pos % 8)) & 1) << j
        assert got == int(codes[row, col]), (row, col)
        assert int(sb[(q * nb + b) * 4 + r]) == int(scales[row, col // 32])
    cf, sf = unpack_mxfp6(packed, sb, nq * 4, k)              # padding: rows past N hold code 0 and scale byte 127
    assert int(cf[n:].sum()) == 0 and bool((sf[n:] == 127).all())


def test_weights_layer_accepts_mxfp6_and_still_refuses_unknown_modes(tiny_cfg):
    """DeviceWeights checks the mode before it touches a device: an unknown string raises the ValueError that names the built modes - 'mxfp6'
    among them; mxfp6 with fp32 matrices raises the bf16 rule, which only an accepted mode reaches; the MXFP4-only keywords refuse it"""
    with pytest.raises(ValueError, match="mxfp6"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant="mxfp8")
    with pytest.raises(ValueError, match="torch_dtype must be bfloat16"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.float32, quant="mxfp6")
    with pytest.raises(ValueError, match="pre-quantized"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant="mxfp6", prequant={"x": object()})
    with pytest.raises(ValueError, match="mxfp4_row_batch"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant="mxfp6", mxfp4_row_batch=True)
    with pytest.raises(ValueError, match="mxfp4_lean"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant="mxfp6", mxfp4_lean=True)


def test_model_keywords_are_checked_before_any_gpu_work(tiny_cfg):
    """row_batch_width=8 and batched_conv_rows=True are refused with weight_quant='mxfp6' as with every quantised mode, and so are the
    MXFP4-only keywords: by the constructor and by from_synthetic, before a weight or a device is touched"""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    for kw, what in ((dict(row_batch_width=8), "row_batch_width=8"), (dict(batched_conv_rows=True), "batched_conv_rows=True"),
                     (dict(mxfp4_row_batch=True), "mxfp4_row_batch"), (dict(mxfp4_lean=True), "mxfp4_lean")):
        with pytest.raises(ValueError, match=what) as ei:
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", **kw)
        assert "mxfp6" in str(ei.value)
        with pytest.raises(ValueError, match=what):
            M.from_synthetic(tiny_cfg, 1, numpy_weights=True, weight_quant="mxfp6", **kw)


def test_device_weights_upload_effective_copies_and_count_the_companions(tiny_cfg, tiny_weights):
    """DeviceWeights(quant='mxfp6'): the descriptors carry VV_WQ_MXFP6, every matrix of fp8_matrix_names with K % 32 == 0 has a companion, the
    bf16 copies hold the effective values, and nbytes() is the bf16 model's plus exactly the companions' bytes: 25 per 32 weights"""
    cfg = tiny_cfg
    w = DeviceWeights(cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp6")
    w0 = DeviceWeights(cfg, tiny_weights, "cpu", torch.bfloat16)
    both = _lib.VV_BF16 | _lib.VV_WQ_MXFP6
    assert (w.llm.wdt, w.head.wdt, w.dec.wdt, w.sem.wdt) == (both,) * 4 and w0.llm.wdt == _lib.VV_BF16 and w.quant == "mxfp6"
    n_q = sum(tiny_weights[name].numel() for name in fp8_matrix_names(cfg) if tiny_weights[name].shape[1] % 32 == 0)
    assert n_q > 0 and all(tiny_weights[name].shape[0] % 4 == 0 for name in fp8_matrix_names(cfg)), "no row padding at these shapes"
    assert w.nbytes() - w0.nbytes() == n_q * 25 // 32
    lay = w.llm.layer[0]
    assert lay.q_qkv.q and lay.q_qkv.scale and lay.q_o.q and lay.q_gate.q and lay.q_up.q and lay.q_down.q
    eff = mxfp6_effective_state_dict(cfg, tiny_weights)
    name = "model.language_model.layers.0.mlp.down_proj.weight"
    held = next(t for t in w._keep if isinstance(t, torch.Tensor) and t.data_ptr() == lay.wdown)
    assert torch.equal(held.float(), eff[name]) and not torch.equal(eff[name], tiny_weights[name].to(torch.bfloat16).float())


def test_effective_state_dict_covers_k_multiples_of_32_only(tiny_cfg):
    names = fp8_matrix_names(tiny_cfg)
    g = torch.Generator().manual_seed(3)
    sd = {name: torch.randn(8, 64 if i % 2 else 48, generator=g).bfloat16() for i, name in enumerate(names)}
    sd["other.weight"] = torch.randn(8, 64, generator=g)
    out = mxfp6_effective_state_dict(tiny_cfg, sd)
    assert set(out) == set(sd) and out["other.weight"] is sd["other.weight"]
    for i, name in enumerate(names):
        if i % 2:
            assert out[name].dtype == torch.float32 and torch.equal(out[name], quantize_mxfp6(sd[name])[2]) and not torch.equal(out[name], sd[name].float())
        else:
            assert out[name] is sd[name], "K % 32 != 0: no companion, the matrix stays as it is"


def test_header_lib_and_docs_agree():
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    assert re.search(r"enum \{ VV_MXFP6 = 6 \};", hdr) and re.search(r"enum \{ VV_WQ_MXFP6 = 0x800 \};", hdr)
    assert (_lib.VV_MXFP6, _lib.VV_WQ_MXFP6, _lib.VV_WQ_FRAG4, _lib.VV_WQ_MXFP4) == (6, 0x800, 0x400, 0x200)
    assert "plane A [4 rows][B blocks][16 B]" in hdr and "[G][B blocks][4 rows]" in hdr and "gemv_mx6<m=2,dual=0,ksplit=5,ku=1>" in hdr
    lib = _lib.load()
    assert lib.vv_abi_version() == 6, "no struct changed: the ABI version stays"
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "mxfp6" in open(os.path.join(ROOT, doc)).read(), doc
    from vibevoice_rocm_amd import build
    assert any(s.endswith("vv_gemv_mx6.hip") for s in build.SRC)
