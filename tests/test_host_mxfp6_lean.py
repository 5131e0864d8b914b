"""mxfp6_lean=True on the host (CPU only): the keyword's validation, what DeviceWeights drops and what it keeps, and that the refusals an mxfp6
model already pins are the same with the keyword.  The MXFP6 image of tests/test_host_mxfp4_lean.py."""
import dataclasses
import os
import re

import pytest
import torch

from conftest import ROOT
from vibevoice_rocm_amd import _lib
from vibevoice_rocm_amd.weights import DeviceWeights


@pytest.mark.parametrize("quant", [None, "fp8", "nf4", "mxfp4"])
def test_keyword_needs_mxfp6(tiny_cfg, quant):
    """another weight_quant raises ValueError before a weight or a device is touched: the model's constructor (an empty state dict is enough),
    from_synthetic through it, and the engine's weights layer"""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    with pytest.raises(ValueError, match="mxfp6_lean"):
        M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=quant, mxfp6_lean=True)
    with pytest.raises(ValueError, match="mxfp6_lean"):
        M.from_synthetic(tiny_cfg, 1, numpy_weights=True, weight_quant=quant, mxfp6_lean=True)
    with pytest.raises(ValueError, match="mxfp6_lean"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant=quant, mxfp6_lean=True)


def test_keyword_is_plumbed_through_every_constructor():
    import inspect
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    for f in (DeviceWeights.__init__, Engine.__init__, M.__init__):
        assert inspect.signature(f).parameters["mxfp6_lean"].default is False, f
    assert 'kw.get("mxfp6_lean", False)' in inspect.getsource(M.from_pretrained)


def test_pinned_refusals_are_unchanged(tiny_cfg):
    """fp32, row_batch_width=8, batched_conv_rows and mxfp4_lean are refused for an mxfp6 model with the keyword exactly as without it"""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    for lean in (False, True):
        with pytest.raises(ValueError, match="torch_dtype must be bfloat16"):
            DeviceWeights(tiny_cfg, {}, "cpu", torch.float32, quant="mxfp6", mxfp6_lean=lean)
        with pytest.raises(ValueError, match="row_batch_width"):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", row_batch_width=8, mxfp6_lean=lean)
        with pytest.raises(ValueError, match="batched_conv_rows"):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", batched_conv_rows=True, mxfp6_lean=lean)
        with pytest.raises(ValueError, match="mxfp4_lean"):
            DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant="mxfp6", mxfp4_lean=True, mxfp6_lean=lean)
        with pytest.raises(ValueError, match="mxfp4_lean"):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", mxfp4_lean=True, mxfp6_lean=lean)
        with pytest.raises(ValueError, match="mxfp4_row_batch"):
            DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant="mxfp6", mxfp4_row_batch=True, mxfp6_lean=lean)
        with pytest.raises(ValueError, match="mxfp6_row_batch"):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="fp8", mxfp6_row_batch=True, mxfp6_lean=False)


def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    assert re.search(r"VV_LIN_PACKED = 16, VV_LIN_W_MXGEMM = 32 \};", hdr)
    assert re.search(r"^enum \{ VV_LIN_W_MX6GEMM = 64 \};$", hdr, re.M)
    assert _lib.LIN_W_MXGEMM == 32 and _lib.LIN_W_MX6GEMM == 64
    assert "There is no lean form" not in hdr and "A LEAN MX LLM (vv_llm with VV_WQ_MXFP4 or VV_WQ_MXFP6)" in hdr


def _weights_of(cfg):
    from vibevoice_rocm_amd.synth import synth_state_dict
    return {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 99).items()}


def _lean_cfg(tiny_cfg):
    return dataclasses.replace(tiny_cfg, hidden=128, inter=256, heads=4, kv_heads=2, head_dim=32)


def test_lean_drops_the_llm_matrices_and_nothing_else(tiny_cfg):
    """A config whose LLM widths the GEMM on the codes takes (hidden 128, inter 256, q width 128, qkv width 256): every LLM matrix is listed,
    its descriptor pointer is NULL beside a present companion, nbytes() falls by exactly the listed bytes, and the head's and the tokenizers'
    matrices keep their bf16 copies.  fork() shares the same descriptors."""
    cfg = _lean_cfg(tiny_cfg)
    sd = _weights_of(cfg)
    w = DeviceWeights(cfg, sd, "cpu", torch.bfloat16, quant="mxfp6", mxfp6_lean=True)
    w0 = DeviceWeights(cfg, sd, "cpu", torch.bfloat16, quant="mxfp6")
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
    for net in (w.dec, w.sem):          # the tokenizers' FFN matrices keep their bf16 copies beside the companions
        for i in range(net.n_stages):
            for j in range(net.n_blocks[i]):
                assert net.blocks[i][j].w1 and net.blocks[i][j].w2
    assert w.llm.wdt == w0.llm.wdt == _lib.VV_BF16 | _lib.VV_WQ_MXFP6
    w.ensure_frag()          # without mxfp6_row_batch there is no bf16 matrix to copy fragment-major: no copy, no failure
    assert all(not w.llm.layer[l].f_qkv for l in range(cfg.layers))


def test_the_companions_of_a_lean_model_hold_the_same_codes(tiny_cfg):
    """the matrix is quantised and packed before the effective matrix is let go: the companion of a lean model is byte for byte the one the model
    with copies holds"""
    cfg = _lean_cfg(tiny_cfg)
    sd = _weights_of(cfg)
    w = DeviceWeights(cfg, sd, "cpu", torch.bfloat16, quant="mxfp6", mxfp6_lean=True)
    w0 = DeviceWeights(cfg, sd, "cpu", torch.bfloat16, quant="mxfp6")

    def by_ptr(ww):
        return {t.data_ptr(): t for t in ww._keep if isinstance(t, torch.Tensor)}

    a, b = by_ptr(w), by_ptr(w0)
    for l in range(cfg.layers):
        for f in ("q_qkv", "q_o", "q_gate", "q_up", "q_down"):
            c, c0 = getattr(w.llm.layer[l], f), getattr(w0.llm.layer[l], f)
            assert torch.equal(a[c.q], b[c0.q]) and torch.equal(a[c.scale], b[c0.scale]), (l, f)
            assert a[c.q].dtype == torch.uint8 and a[c.q].numel() == b[c0.q].numel()


def test_lean_keeps_every_copy_when_a_width_does_not_fit(tiny_cfg, tiny_weights):
    """tiny (hidden 64): no LLM matrix has K % 128 == 0 throughout, and a model is lean as a whole or not at all - nothing is dropped"""
    w = DeviceWeights(tiny_cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp6", mxfp6_lean=True)
    assert w.lean_report() == []
    lay = w.llm.layer[0]
    assert lay.wqkv and lay.wo and lay.wgate and lay.wup and lay.wdown
    assert w.nbytes() == DeviceWeights(tiny_cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp6").nbytes()


def test_one_width_off_keeps_every_copy(tiny_cfg):
    """inter 192 (% 128 != 0) beside widths that fit: the down projection alone could not run on the codes, so every copy is kept"""
    cfg = dataclasses.replace(_lean_cfg(tiny_cfg), inter=192)
    w = DeviceWeights(cfg, _weights_of(cfg), "cpu", torch.bfloat16, quant="mxfp6", mxfp6_lean=True)
    assert w.lean_report() == []
    for l in range(cfg.layers):
        lay = w.llm.layer[l]
        assert lay.wqkv and lay.wo and lay.wgate and lay.wup and lay.wdown


def test_lean_with_row_batch_builds_the_fragment_copies_from_the_companions(tiny_cfg):
    cfg = _lean_cfg(tiny_cfg)
    w = DeviceWeights(cfg, _weights_of(cfg), "cpu", torch.bfloat16, quant="mxfp6", mxfp6_lean=True, mxfp6_row_batch=True)
    assert w.llm.wdt == _lib.VV_BF16 | _lib.VV_WQ_MXFP6 | _lib.VV_WQ_FRAG6
    before = w.nbytes()
    w.ensure_frag()
    for l in range(cfg.layers):
        lay = w.llm.layer[l]
        assert lay.f_qkv and lay.f_o and lay.f_gate and lay.f_up and lay.f_down and not lay.wqkv
    n_llm = sum(d["n"] * d["k"] for d in w.lean_report())
    assert n_llm and w._frag_state["mxfp6_weights"] >= n_llm and w.nbytes() == before + w._frag_state["mxfp6_bytes"]
    assert w._frag_state["mxfp4_weights"] == 0
    # the copies are the companions re-laid: the first layer's qkv copy unpacks to the codes the companion unpacks to
    from vibevoice_rocm_amd.weights import unpack_mxfp6
    keep = {t.data_ptr(): t for t in w._keep if isinstance(t, torch.Tensor)}
    lay = w.llm.layer[0]
    codes, sb = unpack_mxfp6(keep[lay.q_qkv.q], keep[lay.q_qkv.scale], 256, 128)
    frag = next(t for t in w._frag_state["tensors"] if t.data_ptr() == lay.f_qkv)
    c2, s2 = DeviceWeights.unfrag_mxfp6(frag, 256, 128)
    assert torch.equal(codes, c2) and torch.equal(sb, s2)
