"""Weight-only 4-bit NF4 (weight_quant="nf4") on the MI355X: vv_linear's VV_NF4 form on the streaming GEMV against torch on the effective
matrix, generate() and the 7B-shape components against the oracle on nf4_effective_state_dict, graphs, batches on the lanes, the 3..8-row
entry points with the NF4 bit, and the from_pretrained(quantization_config=BitsAndBytesConfig(...)) drop-in call."""
import ctypes as C
import dataclasses

import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

VV_E_ARG, VV_E_UNSUPPORTED = -1, -3      # include/vv_hip.h
REF_QC = dict(load_in_4bit=True, bnb_4bit_quant_type="nf4", bnb_4bit_use_double_quant=True, bnb_4bit_compute_dtype=torch.float16)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    from vibevoice_rocm_amd import _lib
    return _lib


class _Tok:
    def __init__(self, st, se, sd, eos):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = st, se, sd, eos
        self.bos_token_id = None
        self.pad_id = 0


def _nf4_matrix(n, k, g):
    """A [N, K] matrix whose every row holds all 16 codes (block 0) and one all-zero block (block 1 when K >= 128)."""
    from vibevoice_rocm_amd.weights import NF4_TABLE
    w = torch.randn(n, k, generator=g) / k ** 0.5
    w[:, :16] = torch.tensor(NF4_TABLE) * w[:, :64].abs().amax(dim=1, keepdim=True)
    if k >= 128:
        w[:, 64:128] = 0.0
    return w.bfloat16().float()


SHAPES = [(2048, 1536, False), (1536, 1536, False), (8960, 1536, True), (1536, 8960, False), (4608, 1536, True), (8192, 2048, False),
          (2048, 8192, False), (4608, 3584, False), (18944, 3584, True), (3584, 18944, False), (10752, 3584, True), (96, 512, False)]


@pytest.mark.parametrize("variant", ["rms_mod", "silu_gate", "plain_res"])
@pytest.mark.parametrize("m", [1, 2])
@pytest.mark.parametrize("n,k,dual", SHAPES)
def test_linear_nf4_weights(lib, n, k, dual, m, variant):
    """VV_NF4 on the streaming GEMV: codes, block scales and the bf16 rounding of table * absmax, with the prologues (RMSNorm + adaLN modulate,
    SiLU) and epilogues (bias, GELU, SwiGLU, per-row and per-channel gate, residual) against torch on the effective matrix."""
    from vibevoice_rocm_amd.weights import pack_nf4, quantize_nf4
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(7 * m + n + k)
    w, w2 = _nf4_matrix(n, k, g), _nf4_matrix(n, k, g)
    c1, s1, e1 = quantize_nf4(w)
    c2, s2, e2 = quantize_nf4(w2)
    for c in (c1, c2):
        assert all(len(set(c[r, :64].tolist())) == 16 for r in range(n)), "every row must carry all 16 codes"
    if k >= 128:
        assert bool((s1[:, 1] == 0).all()) and bool((c1[:, 64:128] == 7).all())
    p1, q1 = pack_nf4(c1, s1)
    p2, q2 = pack_nf4(c2, s2)
    x = torch.randn(m, k, generator=g)
    nw, sh, sc = 1 + 0.1 * torch.randn(k, generator=g), 0.2 * torch.randn(m, k, generator=g), 0.2 * torch.randn(m, k, generator=g)
    bias, gate_r, gate_v, res = 0.1 * torch.randn(n, generator=g), torch.randn(m, n, generator=g), torch.randn(n, generator=g), torch.randn(m, n, generator=g)
    d = [t.cuda().contiguous() for t in (x, p1, q1, p2, q2, nw, sh, sc, bias, gate_r, gate_v, res)]
    out = torch.full((m, n), float("nan"), device="cuda")
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo = d[0].data_ptr(), k, m, n, k, L.VV_NF4, out.data_ptr(), n
    a.w, a.wscale = d[1].data_ptr(), d[2].data_ptr()
    xd = x.double()
    if variant == "rms_mod":
        a.pro, a.norm_w, a.eps = 1, d[5].data_ptr(), 1e-6
        a.mod_shift, a.mod_scale, a.ld_mod = d[6].data_ptr(), d[7].data_ptr(), k
        xd = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-6) * nw.double()
        xd = xd * (1 + sc.double()) + sh.double()
    elif variant == "silu_gate":
        a.pro = 2
        xd = xd * torch.sigmoid(xd)
    y = xd @ e1.double().T
    if variant != "rms_mod" or not dual:     # the bias enters before the activation (vv_hip.h epilogue order)
        a.bias = d[8].data_ptr()
        y = y + bias.double()
    if dual:
        a.w2, a.w2scale, a.act = d[3].data_ptr(), d[4].data_ptr(), 2
        y = torch.nn.functional.silu(y) * (xd @ e2.double().T)
    elif variant != "plain_res":
        a.act = 1
        y = torch.nn.functional.gelu(y)
    if variant == "silu_gate":
        a.gate, a.gate_ld, a.res, a.ldres = d[9].data_ptr(), n, d[11].data_ptr(), n
        y = y * gate_r.double() + res.double()
    elif variant == "plain_res":
        a.gate, a.gate_ld, a.res, a.ldres = d[10].data_ptr(), 0, d[11].data_ptr(), n
        y = y * gate_v.double() + res.double()
    L.check(l.vv_linear(C.byref(a), None), "vv_linear nf4")
    torch.cuda.synchronize()
    e = rel_rms(out.cpu().numpy(), y.float().numpy())
    assert e < 2e-6, f"nf4 m={m} n={n} k={k} dual={dual} {variant}: rel RMS {e:.3e}"


def test_linear_nf4_rejections(lib):
    """Every NF4 call the streaming GEMV cannot take is an error, never a read of the codes as another type."""
    from vibevoice_rocm_amd.weights import pack_nf4, quantize_nf4
    L = lib
    l = L.load()
    n, k = 256, 1536
    c, s, _ = quantize_nf4(torch.randn(n, k))
    p, q = [t.cuda() for t in pack_nf4(c, s)]
    x = torch.randn(12, 1600, device="cuda")
    out = torch.zeros(12, n, device="cuda")

    def args(m, kk=k):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo = x.data_ptr(), 1600, m, n, kk, L.VV_NF4, out.data_ptr(), n
        a.w, a.wscale = p.data_ptr(), q.data_ptr()
        return a
    assert l.vv_linear(C.byref(args(2)), None) == 0
    for a in (args(3), args(12), args(2, 1568)):
        assert l.vv_linear(C.byref(a), None) in (VV_E_ARG, VV_E_UNSUPPORTED)
    a = args(2)
    a.wscale = None
    assert l.vv_linear(C.byref(a), None) in (VV_E_ARG, VV_E_UNSUPPORTED)
    a = args(4)
    a.flags = L.LIN_W_FRAG
    assert l.vv_linear(C.byref(a), None) in (VV_E_ARG, VV_E_UNSUPPORTED)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# whole model at mid shapes
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("mid")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 4321).items()}
    return cfg, sd


def _special(cfg):
    V = cfg.vocab
    return V - 4, V - 3, V - 2, V - 1


def _gen(m, cfg, ids, forced, noise, steps=10):
    m.set_ddpm_inference_steps(steps)
    return m.generate(input_ids=ids[None], tokenizer=_Tok(*_special(cfg)), cfg_scale=2.0, forced_tokens=forced, noise=noise)


def test_generate_mid_nf4_vs_oracle(mid):
    """weight_quant="nf4": generate() (70-token prompt: prefill on the bf16 copies of the effective weights, decode on the NF4 codes) against
    the oracle on nf4_effective_state_dict; and clearly different from the unquantised model."""
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.weights import fp8_matrix_names, nf4_effective_state_dict
    cfg, sd = mid
    eff = nf4_effective_state_dict(cfg, sd)
    names = set(fp8_matrix_names(cfg))
    sd_o = {k: (eff[k] if k in names else (v.to(torch.bfloat16).float() if v.dim() >= 2 else v)) for k, v in sd.items()}
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg.vocab - 8, (70,), generator=g)
    forced = [ST] + [D] * 5 + [E, EOS]
    noise = torch.randn(5, cfg.latent, generator=g)
    ref = O.generate(sd_o, cfg.as_dict(), ids.tolist(), torch.zeros(70, dtype=torch.bool), None, dict(speech_start=ST, speech_end=E,
                     speech_diffusion=D, eos=EOS), noise, cfg_scale=2.0, n_steps=10, forced_tokens=forced, bf16_t=True)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="nf4")
    out = _gen(m, cfg, ids, forced, noise)
    assert out.sequences[0, 70:].tolist() == forced
    got, want = out.speech_outputs[0][0].cpu().numpy(), torch.cat(ref.audio).numpy()
    assert got.shape == want.shape == (5 * cfg.hop,)
    err = rel_rms(got, want)
    assert err < 2e-2, f"nf4 generate() vs oracle on the effective weights: rel RMS {err:.3e}"
    m2 = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    out2 = _gen(m2, cfg, ids, forced, noise)
    assert rel_rms(out2.speech_outputs[0][0].cpu().numpy(), got) > 5e-2


def test_generate_mid_nf4_graphs_equal_eager(mid):
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg, sd = mid
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(0, cfg.vocab - 8, (24,), generator=g)
    forced = [ST] + [D] * 4 + [E, ST, D, D, E, EOS]
    noise = torch.randn(6, cfg.latent, generator=g)
    outs = []
    for graphs in (False, True):
        m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="nf4", use_graphs=graphs)
        outs.append(_gen(m, cfg, ids, forced, noise).speech_outputs[0].cpu())
    assert torch.equal(outs[0], outs[1]), "nf4: graph replay must equal eager bit for bit"


def test_generate_mid_nf4_batch_of_3_on_lanes(mid):
    """3 nf4 dialogues run on the lock-step lanes (the row-batched path has no NF4) and equal three single-dialogue calls bit for bit."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg, sd = mid
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(13)
    ids = torch.randint(0, cfg.vocab - 8, (3, 20), generator=g)
    forced = [[ST, D, D, D, E, EOS], [ST, D, E, EOS], [ST, D, D, E, ST, D, E, EOS]]
    noise = torch.randn(3, 4, cfg.latent, generator=g)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="nf4")
    m.set_ddpm_inference_steps(10)
    tok = _Tok(ST, E, D, EOS)
    out = m.generate(input_ids=ids, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    assert not m._rowbatch, "nf4 batch took the row-batched path"
    for b in range(3):
        one = m.generate(input_ids=ids[b:b + 1], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[b], noise=noise[b])
        assert torch.equal(one.speech_outputs[0].cpu(), out.speech_outputs[b].cpu()), f"dialogue {b}: lanes != single call"


def test_nf4_bit_on_row_batched_head_sampler(mid):
    """vv_head_sample_batch (2 utterances = 4 rows: the 3..8-row GEMV) on a head descriptor with the NF4 bit never streams the NF4 companions
    through the fp8 fragment path: it equals the same call on a bf16 model built from the effective weights, bit for bit."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.weights import nf4_effective_state_dict
    cfg, sd = mid
    eq = Engine(cfg, sd, device="cuda:0", dtype=torch.bfloat16, use_graphs=False, weight_quant="nf4")
    eb = Engine(cfg, nf4_effective_state_dict(cfg, sd), device="cuda:0", dtype=torch.bfloat16, use_graphs=False)
    assert eq.w.head.wdt == L.VV_BF16 | L.VV_WQ_NF4 and eb.w.head.wdt == L.VV_BF16
    g = torch.Generator().manual_seed(14)
    B = 2
    cond, noise = torch.randn(2 * B, cfg.hidden, generator=g).cuda(), torch.randn(B, cfg.latent, generator=g).cuda()
    res = []
    for eng in (eq, eb):
        eng.w.ensure_frag()
        eng.set_steps(10)
        lb = eng.lib
        with torch.cuda.stream(eng.stream):
            ws = torch.empty(lb.vv_head_ws_bytes_batch(C.byref(eng.w.head), 10, B), dtype=torch.uint8, device="cuda")
            lat = torch.zeros(B, cfg.latent, device="cuda")
            eng._ck(lb.vv_head_sample_batch(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(),
                                            eng._coefs, 10, 2.0, lat.data_ptr(), cfg.latent, B, ws.data_ptr(), eng.sp), "vv_head_sample_batch")
        eng.stream.synchronize()
        res.append(lat.cpu())
    assert torch.isfinite(res[0]).all() and torch.equal(res[0], res[1])


def test_from_pretrained_bnb_config_drop_in(mid, tmp_path):
    """The reference's 4-bit call: from_pretrained(dir, quantization_config=BitsAndBytesConfig(nf4, double quant, fp16 compute),
    torch_dtype=torch.float16) gives weight_quant == "nf4" and the output of a directly built weight_quant="nf4" model, bit for bit."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference, save_checkpoint_dir
    cfg, sd = mid
    save_checkpoint_dir(str(tmp_path), cfg, sd)
    try:
        from transformers import BitsAndBytesConfig
        qc = BitsAndBytesConfig(**REF_QC)
    except Exception:
        qc = dict(REF_QC)
    m = VibeVoiceForConditionalGenerationInference.from_pretrained(str(tmp_path), quantization_config=qc, torch_dtype=torch.float16,
                                                                   device_map="cuda")
    assert m.weight_quant == "nf4" and m.dtype == torch.bfloat16
    m2 = VibeVoiceForConditionalGenerationInference(m.config, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="nf4")
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(15)
    ids = torch.randint(0, cfg.vocab - 8, (20,), generator=g)
    forced = [ST, D, D, D, E, EOS]
    noise = torch.randn(3, cfg.latent, generator=g)
    a, b = _gen(m, m.config, ids, forced, noise), _gen(m2, m.config, ids, forced, noise)
    assert torch.equal(a.speech_outputs[0].cpu(), b.speech_outputs[0].cpu())


# ---------------------------------------------------------------------------------------------------------------
# 7B widths (4 LLM layers: the oracle runs on the CPU)
# ---------------------------------------------------------------------------------------------------------------
def test_7b_components_nf4_vs_oracle():
    """7B widths (H 3584, I 18944, head 3584 / 10752, untied lm_head) with weight_quant="nf4": head sampling (20 steps, CFG 2), prompt
    prefill (80 rows) + batch-2 decode step with the constrained logits, 3 streaming decoder + semantic-encoder frames, against the oracle
    on the effective weights."""
    _need_gpu()
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    from vibevoice_rocm_amd.weights import nf4_effective_state_dict
    cfg = dataclasses.replace(VVConfig.preset("7b"), layers=4)
    sd = synth_state_dict_torch(cfg, 778, device="cuda:0", dtype=torch.bfloat16)
    torch.set_num_threads(16)
    eng = Engine(cfg, sd, device="cuda:0", dtype=torch.bfloat16, use_graphs=False, weight_quant="nf4")
    sd_o = nf4_effective_state_dict(cfg, sd)
    ocfg = cfg.as_dict()
    g = torch.Generator().manual_seed(42)

    def cpu(prefix):
        return {k: v.float().cpu() for k, v in sd_o.items() if k.startswith(prefix)}
    W = cpu("model.prediction_head.")
    cond, ncond, noise = torch.randn(1, cfg.hidden, generator=g), torch.randn(1, cfg.hidden, generator=g), torch.randn(1, cfg.latent, generator=g)
    ref = O.sample_speech_tokens(W, ocfg, cond, ncond, noise, 2.0, 20, bf16_t=True)[0].numpy()
    eng.set_steps(20)
    with torch.cuda.stream(eng.stream):
        eng.hidden2[0].copy_(cond[0].cuda()); eng.hidden2[1].copy_(ncond[0].cuda()); eng.noise_dev.copy_(noise[0].cuda())
        eng._ck(eng.lib.vv_head_sample(C.byref(eng.w.head), eng.hidden2.data_ptr(), cfg.hidden, eng.noise_dev.data_ptr(), eng.temb.data_ptr(),
                                       eng._coefs, 20, 2.0, eng.latent.data_ptr(), eng._head_ws.data_ptr(), None, eng.sp), "vv_head_sample")
    eng.stream.synchronize()
    e = rel_rms(eng.latent.cpu().numpy(), ref)
    assert e < 2e-2, f"7B nf4 head sampling: rel RMS {e:.3e}"
    del W
    W = cpu("model.language_model.")
    W["lm_head.weight"] = sd_o["lm_head.weight"].float().cpu()
    ids = torch.randint(0, 1000, (80,), generator=g)
    emb = W["model.language_model.embed_tokens.weight"]
    kv, nkv = O.KVCache(cfg.layers), O.KVCache(cfg.layers)
    h_ref = O.llm_forward(W, ocfg, emb[ids], kv, 0)[-1]
    O.llm_forward(W, ocfg, emb[ids[:7]], nkv, 0)
    valid = [cfg.vocab - 4, cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1]
    eng.begin_sequence(256, valid)
    eng.prefill(eng.embed_ids(ids), row=0)
    eng.prefill(eng.embed_ids(ids[:7]), row=1)
    eng.stream.synchronize()
    e = rel_rms(eng.hidden2[0].cpu().numpy(), h_ref.numpy())
    assert e < 2e-2, f"7B nf4 prefill(80) last hidden: rel RMS {e:.3e}"
    x = 0.05 * torch.randn(1, cfg.hidden, generator=g)
    p_ref = O.llm_forward(W, ocfg, x, kv, kv.length)[0]
    n_ref = O.llm_forward(W, ocfg, x, nkv, nkv.length)[0]
    with torch.cuda.stream(eng.stream):
        eng.x2[0].copy_(x[0].cuda()); eng.x2[1].copy_(x[0].cuda())
        eng.llm_forward(eng.x2, eng.lens, None, eng.hidden2)
        eng._logits()
    eng.stream.synchronize()
    ep, en = rel_rms(eng.hidden2[0].cpu().numpy(), p_ref.numpy()), rel_rms(eng.hidden2[1].cpu().numpy(), n_ref.numpy())
    assert ep < 2e-2 and en < 2e-2, f"7B nf4 batch-2 decode: positive {ep:.3e} negative {en:.3e}"
    lg_ref = (p_ref @ O.lm_head_weight(W, ocfg)[valid].t()).numpy()
    el = rel_rms(eng.logits[:4].cpu().numpy(), lg_ref)
    assert el < 2e-2, f"7B nf4 constrained logits: rel RMS {el:.3e}"
    del W, kv, nkv
    Wd, Ws = cpu("model.acoustic_tokenizer.decoder."), cpu("model.semantic_tokenizer.encoder.")
    st_d, st_s = O.ConvState(), O.ConvState()
    with torch.cuda.stream(eng.stream):
        eng.reset_speech_caches()
    for f in range(3):
        lat = torch.randn(cfg.ac_dim, generator=g)
        wav_ref = O.tokenizer_decoder(Wd, ocfg, lat[:, None], st_d)[0]
        sem_ref = O.semantic_encode(Ws, ocfg, wav_ref[None], st_s)[0]
        with torch.cuda.stream(eng.stream):
            ld, wr = lat.cuda(), wav_ref.cuda()
            eng._ck(eng.lib.vv_decoder_forward(C.byref(eng.w.dec), ld.data_ptr(), 1, 1.0, 0.0, eng.wav.data_ptr(), eng._dec_ws.data_ptr(), eng.sp), "dec")
            eng._ck(eng.lib.vv_encoder_forward(C.byref(eng.w.sem), wr.data_ptr(), cfg.hop, eng.sem.data_ptr(), eng._sem_ws.data_ptr(), eng.sp), "sem")
        eng.stream.synchronize()
        ed, es = rel_rms(eng.wav.cpu().numpy(), wav_ref.numpy()), rel_rms(eng.sem.cpu().numpy(), sem_ref.numpy())
        assert ed < 2e-2 and es < 2e-2, f"7B nf4 frame {f}: decoder {ed:.3e} semantic {es:.3e}"
    eng.close()
