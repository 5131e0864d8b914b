"""mxfp4_lean=True on the host (CPU only): the keyword's validation, what DeviceWeights drops and what it keeps, and that the refusals an mxfp4
model already pins are the same with the keyword."""
import dataclasses
import os
import re

import pytest
import torch

from conftest import ROOT
from vibevoice_rocm_amd import _lib
from vibevoice_rocm_amd.weights import DeviceWeights


@pytest.mark.parametrize("quant", [None, "fp8", "nf4"])
def test_keyword_needs_mxfp4(tiny_cfg, quant):
    """another weight_quant raises ValueError before a weight or a device is touched: the model's constructor (an empty state dict is enough),
    from_synthetic through it, and the engine's weights layer"""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    with pytest.raises(ValueError, match="mxfp4_lean"):
        M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=quant, mxfp4_lean=True)
    with pytest.raises(ValueError, match="mxfp4_lean"):
        M.from_synthetic(tiny_cfg, 1, numpy_weights=True, weight_quant=quant, mxfp4_lean=True)
    with pytest.raises(ValueError, match="mxfp4_lean"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant=quant, mxfp4_lean=True)


def test_pinned_refusals_are_unchanged(tiny_cfg):
    """fp32, row_batch_width=8 and batched_conv_rows are refused for an mxfp4 model with the keyword exactly as without it"""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    for lean in (False, True):
        with pytest.raises(ValueError, match="torch_dtype must be bfloat16"):
            DeviceWeights(tiny_cfg, {}, "cpu", torch.float32, quant="mxfp4", mxfp4_lean=lean)
        with pytest.raises(ValueError, match="row_batch_width"):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp4", row_batch_width=8, mxfp4_lean=lean)
        with pytest.raises(ValueError, match="batched_conv_rows"):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp4", batched_conv_rows=True, mxfp4_lean=lean)
        with pytest.raises(ValueError, match="mxfp4_row_batch"):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="fp8", mxfp4_row_batch=True, mxfp4_lean=False)


def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    assert re.search(r"VV_LIN_PACKED = 16, VV_LIN_W_MXGEMM = 32 \};", hdr)
    assert _lib.LIN_W_MXGEMM == 32


def _weights_of(cfg):
    from vibevoice_rocm_amd.synth import synth_state_dict
    return {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 99).items()}


def test_lean_drops_the_llm_matrices_and_nothing_else(tiny_cfg):
    """A config whose LLM widths the GEMM on the codes takes (hidden 128, inter 256, q width 128, qkv width 256): every LLM matrix is listed,
    its descriptor pointer is NULL beside a present companion, nbytes() falls by exactly the listed bytes, and the head's and the tokenizers'
    matrices keep their bf16 copies.  fork() shares the same descriptors."""
    cfg = dataclasses.replace(tiny_cfg, hidden=128, inter=256, heads=4, kv_heads=2, head_dim=32)
    sd = _weights_of(cfg)
    w = DeviceWeights(cfg, sd, "cpu", torch.bfloat16, quant="mxfp4", mxfp4_lean=True)
    w0 = DeviceWeights(cfg, sd, "cpu", torch.bfloat16, quant="mxfp4")
    rep = w.lean_report()
    want = {}
    for l in range(cfg.layers):
        q = f"model.language_model.layers.{l}."
        want.update({q + "self_attn.qkv_proj.weight": (256, 128), q + "self_attn.o_proj.weight": (128, 128), q + "mlp.gate_proj.weight": (256, 128),
                     q + "mlp.up_proj.weight": (256, 128), q + "mlp.down_proj.weight": (128, 256)})
    assert {d["name"]: (d["n"], d["k"]) for d in rep} == want
    assert all(d["bytes"] == 2 * d["n"] * d["k"] for d in rep)
    assert w0.lean_report() == [] and w.nbytes() == w0.nbytes() - sum(d["bytes"] for d in rep)
    for ww in (w, w.fork()):
        for l in range(cfg.layers):
            lay = ww.llm.layer[l]
            assert not (lay.wqkv or lay.wo or lay.wgate or lay.wup or lay.wdown)
            assert all(c.q and c.scale for c in (lay.q_qkv, lay.q_o, lay.q_gate, lay.q_up, lay.q_down))
    for l in range(cfg.head_layers):
        lay = w.head.layer[l]
        assert lay.wgate and lay.wup and lay.wdown and lay.q_gate.q
    assert w.llm.wdt == w0.llm.wdt == _lib.VV_BF16 | _lib.VV_WQ_MXFP4
    w.ensure_frag()          # without mxfp4_row_batch there is no bf16 matrix to copy fragment-major: no copy, no failure
    assert all(not w.llm.layer[l].f_qkv for l in range(cfg.layers))


def test_lean_keeps_every_copy_when_a_width_does_not_fit(tiny_cfg, tiny_weights):
    """tiny (hidden 64): no LLM matrix has K % 128 == 0 throughout, and a model is lean as a whole or not at all - nothing is dropped"""
    w = DeviceWeights(tiny_cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp4", mxfp4_lean=True)
    assert w.lean_report() == []
    lay = w.llm.layer[0]
    assert lay.wqkv and lay.wo and lay.wgate and lay.wup and lay.wdown
    assert w.nbytes() == DeviceWeights(tiny_cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp4").nbytes()


def test_lean_with_row_batch_builds_the_fragment_copies_from_the_companions(tiny_cfg):
    cfg = dataclasses.replace(tiny_cfg, hidden=128, inter=256, heads=4, kv_heads=2, head_dim=32)
    w = DeviceWeights(cfg, _weights_of(cfg), "cpu", torch.bfloat16, quant="mxfp4", mxfp4_lean=True, mxfp4_row_batch=True)
    before = w.nbytes()
    w.ensure_frag()
    for l in range(cfg.layers):
        lay = w.llm.layer[l]
        assert lay.f_qkv and lay.f_o and lay.f_gate and lay.f_up and lay.f_down and not lay.wqkv
    n_llm = sum(d["n"] * d["k"] for d in w.lean_report())
    assert w._frag_state["mxfp4_weights"] >= n_llm and w.nbytes() == before + w._frag_state["mxfp4_bytes"]
