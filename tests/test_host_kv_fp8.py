"""CPU-only checks of the optional fp8 (e4m3) KV cache: the `kv_cache_dtype` option is validated before anything touches a GPU, the scale rule
of vv_kv_quantize as a pure function against hand values, and the vv_kv mirror (two new device pointers, the new entry points)."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT


def test_kv_cache_dtype_is_validated_before_any_gpu_work():
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.engine import check_kv_cache_dtype
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    assert check_kv_cache_dtype(None, torch.bfloat16, 128) is False
    assert check_kv_cache_dtype("bf16", torch.bfloat16, 128) is False
    assert check_kv_cache_dtype(None, torch.float32, 16) is False
    assert check_kv_cache_dtype("fp8", torch.bfloat16, 128) is True
    for bad in ("int8", "fp8_e5m2", "FP8", ""):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            check_kv_cache_dtype(bad, torch.bfloat16, 128)
    with pytest.raises(ValueError, match="bfloat16"):
        check_kv_cache_dtype("fp8", torch.float32, 128)
    with pytest.raises(ValueError, match="head_dim"):
        check_kv_cache_dtype("fp8", torch.bfloat16, 16)
    # the public constructors: the ValueError comes first (no state dict, no GPU needed to get it)
    mid, tiny = VVConfig.preset("mid"), VVConfig.preset("tiny")
    assert mid.head_dim == 128 and tiny.head_dim != 128
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        M(mid, {}, kv_cache_dtype="int4")
    with pytest.raises(ValueError, match="bfloat16"):
        M(mid, {}, torch_dtype=torch.float32, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="head_dim"):
        M(tiny, {}, torch_dtype=torch.bfloat16, kv_cache_dtype="fp8")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        M.from_synthetic(mid, numpy_weights=True, kv_cache_dtype="e4m3")


def test_scale_rule_hand_values():
    """scale = 2^ceil(log2(absmax / 224)): 2x headroom under e4m3's 448; an all-zero head gets 1."""
    from vibevoice_rocm_amd._lib import kv_fp8_scale
    hand = {0.0: 1.0, 224.0: 1.0, 225.0: 2.0, 448.0: 2.0, 449.0: 4.0, 112.0: 0.5, 113.0: 1.0, 1.0: 2.0 ** -7, 1.75: 2.0 ** -7, 1.7578125: 2.0 ** -6,
            0.875: 2.0 ** -8, 28.0: 0.125, 3.0e4: 256.0, -225.0: 2.0}
    for a, want in hand.items():
        assert kv_fp8_scale(a) == want, (a, kv_fp8_scale(a), want)
    # against the formula itself, over every positive finite bf16 magnitude in a wide range (a bf16 absmax is what the kernel sees)
    import math
    bits = torch.arange(0x3000, 0x5000, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).double().tolist()
    for a in bits:
        s = kv_fp8_scale(a)
        assert s == 2.0 ** math.ceil(math.log2(a / 224.0)), a
        assert a / s <= 224.0 < 2 * a / s or a / s == 224.0      # the largest code magnitude lies in (112, 224]


def test_vv_kv_mirror_and_new_entry_points():
    from vibevoice_rocm_amd import _lib
    names = [f[0] for f in _lib.KV._fields_]
    assert names == ["k", "v", "kvdt", "layers", "rows", "kv_heads", "s_max", "head_dim", "vt", "kscale", "vscale"]
    assert C.sizeof(_lib.KV) == 64 and _lib.KV.kscale.offset == 48 and _lib.KV.vscale.offset == 56
    kv = _lib.KV()
    assert kv.kscale is None and kv.vscale is None, "a default-constructed vv_kv has no scales (fp32 / bf16 caches ignore them)"
    for fn in ("vv_kv_quantize", "vv_attn_decode_split", "vv_attn_decode_part_floats"):
        assert fn in _lib.PROTOTYPES
    assert _lib.PROTOTYPES["vv_kv_quantize"][1][:2] == [C.POINTER(_lib.KV), C.POINTER(_lib.KV)] and len(_lib.PROTOTYPES["vv_kv_quantize"][1]) == 7
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    body = re.search(r"typedef struct vv_kv \{(.*?)\} vv_kv;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body)[-2:] == ["kscale", "vscale"], "the scale pointers are the last two fields of vv_kv"
    lib = _lib.load()                      # struct sizes are checked against the library inside
    assert lib.vv_sizeof(b"vv_kv") == C.sizeof(_lib.KV)
    assert lib.vv_attn_decode_part_floats(2, 12, 4) == 2 * 12 * 4 * 130
