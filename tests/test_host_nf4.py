"""Weight-only 4-bit NF4 (weight_quant="nf4") on the host: the quantiser's definition (bitsandbytes' blockwise NF4 restated), the packed layout
of the streaming GEMV, the effective state dict, and the from_pretrained(quantization_config=...) mapping.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.weights import (NF4_TABLE, fp8_matrix_names, nf4_effective_state_dict, pack_nf4, quantize_nf4,
                                        unpack_nf4)

BNB_TABLE = [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
             -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
             0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0]


def _table32():
    return torch.tensor(BNB_TABLE, dtype=torch.float32)


def test_table_values_and_order():
    assert list(NF4_TABLE) == BNB_TABLE
    assert all(a < b for a, b in zip(BNB_TABLE, BNB_TABLE[1:])) and BNB_TABLE[7] == 0.0


def test_nearest_code_on_random_data():
    g = torch.Generator().manual_seed(3)
    w = torch.randn(16, 512, generator=g)
    codes, absmax, _ = quantize_nf4(w)
    x = (w.reshape(16, 8, 64) * torch.reciprocal(absmax)[..., None]).reshape(16, 512)
    d = (x[..., None] - _table32()).abs()                       # distance to every entry
    best = d.min(dim=-1).values
    assert torch.equal(d.gather(-1, codes.long()[..., None])[..., 0], best), "a code is not the nearest table entry"


@pytest.mark.parametrize("i", range(15))
def test_midpoints_plus_minus_one_ulp(i):
    """At bnb's thresholds (midpoints of neighbouring entries as fp32 constants): one ulp above takes the upper code, the midpoint itself and
    one ulp below the lower one (dQuantizeNF4 compares x > threshold)."""
    mid = np.float32((np.float64(BNB_TABLE[i]) + np.float64(BNB_TABLE[i + 1])) / 2)
    vals = [np.nextafter(mid, np.float32(-2)), mid, np.nextafter(mid, np.float32(2))]
    w = torch.zeros(1, 64)
    w[0, 0] = 1.0                                                # absmax 1: x == w exactly
    w[0, 1:4] = torch.tensor(np.array(vals, dtype=np.float32))
    codes, absmax, _ = quantize_nf4(w)
    assert float(absmax[0, 0]) == 1.0
    assert codes[0, 1:4].tolist() == [i, i, i + 1]


def test_blocks_are_per_row_per_64():
    g = torch.Generator().manual_seed(4)
    w = torch.randn(6, 320, generator=g) * 0.02
    _, a0, _ = quantize_nf4(w)
    w2 = w.clone()
    w2[3, 130] = 50.0                                            # row 3, block 2
    c2, a2, _ = quantize_nf4(w2)
    changed = (a0 != a2).nonzero().tolist()
    assert changed == [[3, 2]] and float(a2[3, 2]) == 50.0
    assert int(c2[3, 130]) == 15


def test_zero_block_code7_scale0_no_nan():
    w = torch.randn(2, 192)
    w[1, 64:128] = 0.0
    codes, absmax, eff = quantize_nf4(w)
    assert float(absmax[1, 1]) == 0.0 and bool((codes[1, 64:128] == 7).all())
    assert torch.isfinite(eff).all() and bool((eff[1, 64:128] == 0).all())


def test_effective_weights_are_bf16_of_table_times_absmax():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(32, 1024, generator=g) * 0.05).bfloat16()
    codes, absmax, eff = quantize_nf4(w)
    assert torch.equal(eff.bfloat16().float(), eff), "effective weights must be exact in bf16"
    want = (_table32()[codes.long()] * absmax.repeat_interleave(64, dim=1)).bfloat16().float()
    assert torch.equal(eff, want)
    assert set(codes.unique().tolist()) == set(range(16))


@pytest.mark.parametrize("n,k", [(4, 512), (96, 512), (7, 1536), (5, 8960), (3, 18944), (8, 3584), (12, 64)])
def test_pack_unpack_roundtrip(n, k):
    g = torch.Generator().manual_seed(n * k)
    codes = torch.randint(0, 16, (n, k), generator=g, dtype=torch.uint8)
    absmax = torch.rand(n, k // 64, generator=g)
    packed, scales = pack_nf4(codes, absmax)
    nq, ku = (n + 3) // 4, (k + 511) // 512
    assert packed.dtype == torch.uint8 and packed.numel() == nq * ku * 1024 and scales.numel() == nq * ku * 32
    c2, a2 = unpack_nf4(packed, scales, n, k)
    assert torch.equal(c2, codes) and torch.equal(a2, absmax)
    # the layout itself (include/vv_hip.h): code (4 q + r, 512 u + 8 l + i) is nibble i of dword r of lane l's 16 bytes
    q, r, u, l, i = (n - 1) // 4, (n - 1) % 4, (k - 1) // 512, ((k - 1) % 512) // 8, (k - 1) % 8
    if 4 * q + r < n:
        byte = int(packed[((q * ku + u) * 64 + l) * 16 + 4 * r + i // 2])
        assert (byte >> (4 * (i % 2))) & 15 == int(codes[4 * q + r, k - 1])
    assert float(scales[((q * ku + u) * 4 + r) * 8 + ((k - 1) % 512) // 64]) == float(absmax[n - 1, (k - 1) // 64])


def test_effective_state_dict_touches_exactly_the_companion_matrices():
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("tiny")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 5).items()}
    eff = nf4_effective_state_dict(cfg, sd)
    names = {n for n in fp8_matrix_names(cfg) if sd[n].shape[1] % 64 == 0}
    changed = {k for k in sd if not torch.equal(sd[k], eff[k])}
    assert changed == names and names


class _Cfg:     # attribute form of a BitsAndBytesConfig
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _ref_kwargs():
    return dict(load_in_4bit=True, bnb_4bit_quant_type="nf4", bnb_4bit_use_double_quant=True, bnb_4bit_compute_dtype=torch.float16)


def test_quantization_config_mapping():
    from vibevoice_rocm_amd.modeling import weight_quant_from_config
    assert weight_quant_from_config(None) is None and weight_quant_from_config(None, "fp8") == "fp8"
    assert weight_quant_from_config(_ref_kwargs()) == "nf4"
    assert weight_quant_from_config(_Cfg(**_ref_kwargs())) == "nf4"
    assert weight_quant_from_config(dict(_ref_kwargs(), bnb_4bit_compute_dtype=torch.bfloat16), "nf4") == "nf4"
    try:
        from transformers import BitsAndBytesConfig
    except Exception:
        BitsAndBytesConfig = None
    if BitsAndBytesConfig is not None:
        assert weight_quant_from_config(BitsAndBytesConfig(**_ref_kwargs())) == "nf4"


@pytest.mark.parametrize("bad", [dict(load_in_4bit=True, bnb_4bit_quant_type="fp4"), dict(load_in_4bit=True), dict(load_in_8bit=True)])
def test_quantization_config_rejects_fp4_and_8bit(bad):
    from vibevoice_rocm_amd.modeling import weight_quant_from_config
    with pytest.raises(NotImplementedError, match="nf4"):
        weight_quant_from_config(bad)


def test_quantization_config_conflicting_weight_quant():
    from vibevoice_rocm_amd.modeling import weight_quant_from_config
    with pytest.raises(ValueError):
        weight_quant_from_config(_ref_kwargs(), "fp8")


def test_prequantized_bnb_checkpoint_is_refused(tmp_path):
    from safetensors.torch import save_file

    from vibevoice_rocm_amd.modeling import load_state_dict_from_dir
    name = "model.language_model.layers.0.mlp.down_proj.weight"
    save_file({name: torch.zeros(64, 1, dtype=torch.uint8), name + ".absmax": torch.ones(2), name + ".quant_map": torch.tensor(BNB_TABLE),
               name + ".quant_state.bitsandbytes__nf4": torch.zeros(8, dtype=torch.uint8)}, os.path.join(tmp_path, "model.safetensors"))
    with open(os.path.join(tmp_path, "config.json"), "w") as f:
        json.dump({}, f)
    with pytest.raises(NotImplementedError, match="pre-quantized"):
        load_state_dict_from_dir(str(tmp_path))


def test_device_weights_nf4_needs_bf16():
    from vibevoice_rocm_amd.weights import DeviceWeights
    with pytest.raises(ValueError, match="bfloat16"):
        DeviceWeights(VVConfig.preset("tiny"), {}, "cpu", torch.float32, quant="nf4")
    with pytest.raises(ValueError, match="nf4"):
        DeviceWeights(VVConfig.preset("tiny"), {}, "cpu", torch.bfloat16, quant="int4")
