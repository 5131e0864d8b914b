"""Pre-quantized bitsandbytes NF4 checkpoints on the host: the on-disk format (nibble order, block scales, double quantisation, blocks that
straddle rows, odd sizes), the quant-state parse, the refusals, the loader split and the configuration_vibevoice shim.  No GPU."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from bnb_ckpt import bnb_tensors, quant_state_tensor, write_bnb_dir
from vibevoice_rocm_amd import bnb
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.weights import NF4_TABLE

NAME = "model.language_model.layers.0.mlp.down_proj.weight"


def _record(sd):
    plain, recs = bnb.split_prequantized(sd)
    assert list(recs) == [NAME] and not plain
    return recs[NAME]


def _hand_sd(packed, absmax, shape, blocksize, nested=None):
    sd = {NAME: torch.tensor(packed, dtype=torch.uint8).view(-1, 1), NAME + ".quant_map": torch.tensor(NF4_TABLE, dtype=torch.float32)}
    state = {"quant_type": "nf4", "blocksize": blocksize, "dtype": "float16", "shape": list(shape)}
    if nested is None:
        sd[NAME + ".absmax"] = torch.tensor(absmax, dtype=torch.float32)
    else:
        nmap, nabs, nbs, off = nested
        sd[NAME + ".absmax"] = torch.tensor(absmax, dtype=torch.uint8)
        sd[NAME + ".nested_absmax"] = torch.tensor(nabs, dtype=torch.float32)
        sd[NAME + ".nested_quant_map"] = nmap
        state.update(nested_blocksize=nbs, nested_dtype="float32", nested_offset=off)
    sd[NAME + ".quant_state.bitsandbytes__nf4"] = quant_state_tensor(state)
    return sd


def test_nibble_order_high_first():
    """Byte 0xF0 holds code 15 (+1.0) in its high nibble = element 0 and code 0 (-1.0) in its low nibble = element 1."""
    r = _record(_hand_sd([0xF0], [2.0], (1, 2), 64))
    assert bnb.codes(r).tolist() == [15, 0]
    assert bnb.dequantize(r).tolist() == [[2.0, -2.0]]
    r = _record(_hand_sd([0x7F, 0x8E], [0.5], (2, 2), 64))
    assert bnb.codes(r).tolist() == [7, 15, 8, 14]
    assert bnb.dequantize(r).tolist() == [[0.0, 0.5], [float(torch.tensor(NF4_TABLE[8] * 0.5).bfloat16()), float(torch.tensor(NF4_TABLE[14] * 0.5).bfloat16())]]


def test_nested_scales_by_hand():
    """absmax[b] = (map[code_b] * nested_absmax[b // nested_blocksize]) + offset: map values 0.75 / 1.0, nested blocks of 2."""
    nmap = torch.zeros(256)
    nmap[3], nmap[5] = 0.75, 1.0
    r = _record(_hand_sd([0xFF, 0xFF, 0xFF], [3, 5, 3], (3, 2), 2, nested=(nmap, [0.5, 0.25], 2, 0.125)))
    assert r.nested and r.nested_blocksize == 2 and r.nested_offset == 0.125
    assert bnb.block_absmax(r).tolist() == [0.5, 0.625, 0.3125]           # 0.75*0.5+0.125, 1.0*0.5+0.125, 0.75*0.25+0.125
    assert bnb.dequantize(r).tolist() == [[0.5, 0.5], [0.625, 0.625], [0.3125, 0.3125]]


def test_nested_scales_two_roundings():
    """The product and the offset are rounded apart (fp32), not as one fused multiply-add."""
    g = torch.Generator().manual_seed(1)
    nmap = torch.rand(256, generator=g) * 2 - 1
    codes = torch.randint(0, 256, (40,), generator=g, dtype=torch.uint8)
    nabs = torch.rand(3, generator=g) + 0.5
    off = 0.0123456789
    r = _record(_hand_sd([0x12] * 40, codes.tolist(), (8, 10), 2, nested=(nmap, nabs.tolist(), 16, off)))
    want = [np.float32(np.float32(nmap[int(c)]) * np.float32(nabs[b // 16])) + np.float32(off) for b, c in enumerate(codes.tolist())]
    assert bnb.block_absmax(r).tolist() == [float(np.float32(v)) for v in want]


def _scalar_restatement(packed, absmax, n, k, bs):
    out = []
    for j in range(n * k):
        byte = packed[j // 2]
        code = byte >> 4 if j % 2 == 0 else byte & 15
        out.append(np.float32(NF4_TABLE[code]) * np.float32(absmax[j // bs]))
    return torch.tensor(np.array(out, dtype=np.float32)).to(torch.bfloat16).float().view(n, k)


@pytest.mark.parametrize("n,k,bs", [(3, 5, 4), (5, 7, 8), (4, 96, 64), (3, 33, 16), (1, 1, 64)])
def test_straddling_odd_and_partial_blocks(n, k, bs):
    """Blocks run over the flattened weight (they cross rows when K % blocksize != 0), the last byte of an odd N*K is half used and the
    last block may be partial: every element against a scalar restatement."""
    g = torch.Generator().manual_seed(n * 100 + k)
    nb = -(-(n * k) // bs)
    packed = torch.randint(0, 256, (-(-(n * k) // 2),), generator=g).tolist()
    absmax = (torch.rand(nb, generator=g) + 0.1).tolist()
    r = _record(_hand_sd(packed, absmax, (n, k), bs))
    assert r.nblocks == nb and r.k == k and r.n == n
    assert torch.equal(bnb.dequantize(r), _scalar_restatement(packed, absmax, n, k, bs))


def test_writer_roundtrip_through_the_format():
    """The test-side writer's checkpoint decodes to bf16 of the table values times its block absmax (the definition, end to end)."""
    g = torch.Generator().manual_seed(2)
    w = torch.randn(6, 100, generator=g)
    for double in (False, True):
        r = _record(bnb_tensors(NAME, w, blocksize=64, double=double))
        assert r.shape == (6, 100) and r.nested == double and not r.companion_exact()
        eff = bnb.dequantize(r)
        assert torch.equal(eff.bfloat16().float(), eff)
        assert float((eff - w).abs().max()) < 0.5 * float(w.abs().max())


def test_quant_state_parse():
    state = {"quant_type": "nf4", "blocksize": 64, "dtype": "float16", "shape": [4, 128], "nested_blocksize": 256, "nested_dtype": "float32",
             "nested_offset": 0.0314}
    assert bnb.parse_quant_state(quant_state_tensor(state)) == state
    r = _record(bnb_tensors(NAME, torch.randn(4, 128), blocksize=128, double=True))
    assert (r.blocksize, r.nested_blocksize, r.dtype, r.shape) == (128, 256, "float16", (4, 128)) and r.companion_exact()
    assert r.absmax.dtype == torch.uint8 and r.nested_absmax.numel() == 1 and r.nested_quant_map.numel() == 256
    with pytest.raises(ValueError, match="uint8"):
        bnb.parse_quant_state(torch.zeros(4))


def test_companion_condition():
    for bs, k, ok in ((64, 512, True), (128, 512, True), (256, 512, True), (32, 512, False), (64, 96, False), (512, 256, False)):
        r = _record(bnb_tensors(NAME, torch.randn(2, k), blocksize=bs))
        assert r.companion_exact() == ok, (bs, k)


def test_refuses_fp4():
    sd = bnb_tensors(NAME, torch.randn(4, 64))
    st = bnb.parse_quant_state(sd[NAME + ".quant_state.bitsandbytes__nf4"])
    st["quant_type"] = "fp4"
    fp4 = {k: v for k, v in sd.items() if "quant_state" not in k}
    fp4[NAME + ".quant_state.bitsandbytes__fp4"] = quant_state_tensor(st)
    with pytest.raises(NotImplementedError, match="fp4"):
        bnb.split_prequantized(fp4)
    sd[NAME + ".quant_state.bitsandbytes__nf4"] = quant_state_tensor(st)
    with pytest.raises(NotImplementedError, match="fp4"):
        bnb.split_prequantized(sd)


def test_refuses_foreign_quant_map():
    sd = bnb_tensors(NAME, torch.randn(4, 64))
    sd[NAME + ".quant_map"] = torch.linspace(-1, 1, 16)
    with pytest.raises(ValueError, match="quant_map"):
        bnb.split_prequantized(sd)


@pytest.mark.parametrize("drop", [".absmax", ".quant_map", ".nested_absmax", ".nested_quant_map", ""])
def test_refuses_missing_keys(drop):
    sd = bnb_tensors(NAME, torch.randn(4, 64), double=True)
    del sd[NAME + drop]
    with pytest.raises(ValueError, match="missing"):
        bnb.split_prequantized(sd)


def test_refuses_stray_companions_and_storage():
    sd = bnb_tensors(NAME, torch.randn(4, 64))
    del sd[NAME + ".quant_state.bitsandbytes__nf4"]
    with pytest.raises(ValueError, match="without a quant_state"):
        bnb.split_prequantized(sd)
    sd = bnb_tensors(NAME, torch.randn(4, 64))
    sd[NAME] = sd[NAME].to(torch.int8)
    with pytest.raises(ValueError, match="quant_storage"):
        bnb.split_prequantized(sd)
    sd = bnb_tensors(NAME, torch.randn(4, 64))
    sd[NAME] = sd[NAME][:-1]
    with pytest.raises(ValueError, match="packed bytes"):
        bnb.split_prequantized(sd)


def test_refuses_wrong_shape():
    r = _record(bnb_tensors(NAME, torch.randn(4, 64)))
    with pytest.raises(ValueError, match="disagrees"):
        bnb.check_shapes({NAME: r}, {NAME: (64, 4)})
    bnb.check_shapes({NAME: r}, {NAME: (4, 64)})


@pytest.fixture(scope="module")
def tiny():
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("tiny")
    return cfg, {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 7).items()}


def test_loader_split_follows_the_file(tiny, tmp_path):
    from vibevoice_rocm_amd.modeling import load_prequantized_dir, load_state_dict_from_dir
    cfg, sd = tiny
    names = write_bnb_dir(tmp_path, cfg, sd, which="companion", blocksize=64, double=True, rest_dtype=torch.float16)
    plain, recs = load_prequantized_dir(str(tmp_path))
    assert set(recs) == set(names) and not set(plain) & set(names)
    assert set(plain) | set(recs) == set(sd) and all(v.dtype == torch.float16 for v in plain.values() if v.is_floating_point())
    for n in names:
        assert recs[n].shape == tuple(sd[n].shape) and recs[n].nested
    with pytest.raises(NotImplementedError, match="pre-quantized") as e:
        load_state_dict_from_dir(str(tmp_path))
    assert "load_prequantized_dir" in str(e.value)
    plain2, recs2 = load_prequantized_dir(str(_plain_dir(tmp_path, cfg, sd)))
    assert not recs2 and set(plain2) == set(sd)


def _plain_dir(tmp_path, cfg, sd):
    from vibevoice_rocm_amd.modeling import save_checkpoint_dir
    d = tmp_path / "plain"
    save_checkpoint_dir(str(d), cfg, sd)
    return d


def test_from_pretrained_refusals_before_the_device(tiny, tmp_path):
    """fp8 with a pre-quantized directory and a config whose shapes disagree with the file are refused before anything touches a GPU."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    cfg, sd = tiny
    write_bnb_dir(tmp_path, cfg, sd, which="all", blocksize=64)
    with pytest.raises(ValueError, match="fp8"):
        M.from_pretrained(str(tmp_path), weight_quant="fp8")
    wrong = dataclasses.replace(cfg, inter=cfg.inter * 2)
    with pytest.raises(ValueError, match="disagrees"):
        M.from_pretrained(str(tmp_path), config=wrong)
    with pytest.raises(OSError):
        M.from_pretrained(str(tmp_path), subfolder="4bit")


def test_configuration_vibevoice_roundtrip(tiny, tmp_path):
    from vibevoice.modular.configuration_vibevoice import VibeVoiceConfig
    cfg, sd = tiny
    d = _plain_dir(tmp_path, cfg, sd)
    with open(os.path.join(d, "config.json")) as f:
        j = json.load(f)
    c = VibeVoiceConfig.from_pretrained(str(d), cache_dir=None, local_files_only=True)
    assert isinstance(c, VVConfig) and c.to_dict() == j
    assert dataclasses.asdict(c) == dataclasses.asdict(VVConfig.from_pretrained(str(d)))
    assert VVConfig.from_json_dict(c.to_dict()) == VVConfig.from_pretrained(str(d))
    c2 = VibeVoiceConfig(**cfg.as_dict())
    assert VVConfig.from_json_dict(c2.to_dict()) == cfg
