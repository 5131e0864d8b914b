"""GPU parity of weight-only fp8 (weight_quant="fp8") on the row-batched decode path: the 3..8-row matrix-core GEMV on fp8 fragment-major
codes against the same kernel on the bf16 effective matrix (bit for bit) and fp64 torch, its rejections, the batched composites against their
single-dialogue fp8 forms, generate() dispatch, row-batched against the fp8 lanes and the CPU oracle, and the fragment copies built once per
process.  Measured errors go into the parity record (conftest.rel_rms `what=`)."""
import ctypes as C

import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

N_STEPS = 20
# e4m3fn codes the test matrices must contain: +-448 (the largest finite), subnormals (smallest, largest, negative), zero, the smallest normal
SPECIAL_CODES = [0x7E, 0xFE, 0x01, 0x81, 0x07, 0x87, 0x00, 0x08]
# shapes whose K split differs between the two forms: the bf16 launcher gives each wave an ODD number of 32-wide k steps (9 for the 8960-long
# rows, 7 for the 3584-long dual rows), which 64-wide fp8 loads cannot reproduce - the fp8 form sums the same products over other K slices
SPLIT_DIFFERS = {(1536, 8960), (18944, 3584)}


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    lb = L.load()
    L.check(lb.vv_init(), "vv_init")
    return lb


@pytest.fixture(scope="module")
def big8():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset("1.5b")
    sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="fp8")
    m.set_ddpm_inference_steps(N_STEPS)
    return cfg, sd, m


class _Tok:
    def __init__(self, vocab):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = vocab - 4, vocab - 3, vocab - 2, vocab - 1
        self.bos_token_id = None
        self.pad_id = vocab - 5


def _quantised(n, k, seed):
    """e4m3 codes [n, k] with power-of-two row scales (quantize_e4m3_pow2) and SPECIAL_CODES planted in every row; returns (codes, scale, the
    effective matrix code * scale in bf16 - exact)"""
    from vibevoice_rocm_amd.weights import quantize_e4m3_pow2
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = torch.randn(n, k, device="cuda", generator=g) / k ** 0.5
    codes, scale, _ = quantize_e4m3_pow2(w)
    cols = torch.arange(0, k, 37, device="cuda")
    sp = torch.tensor(SPECIAL_CODES, dtype=torch.uint8, device="cuda")
    rows = torch.arange(n, device="cuda")[:, None]
    codes[rows, cols[None, :]] = sp[(rows + torch.arange(cols.numel(), device="cuda")[None, :]) % len(SPECIAL_CODES)]
    eff = codes.view(torch.float8_e4m3fn).float() * scale[:, None]
    eff16 = eff.bfloat16()
    assert torch.equal(eff16.float(), eff), "code * power-of-two scale must be exact in bf16"
    return codes.contiguous(), scale.contiguous(), eff16


def _run(lib, a):
    from vibevoice_rocm_amd import _lib as L
    L.check(lib.vv_linear(C.byref(a), torch.cuda.current_stream().cuda_stream), "vv_linear")


@pytest.mark.parametrize("m_rows", [4, 5, 8])
@pytest.mark.parametrize("shape", [(4608, 1536, True, 1, True, False), (1536, 4608, False, 0, False, True), (2048, 1536, False, 1, False, False),
                                   (1536, 1536, False, 0, False, True), (8960, 1536, True, 1, False, False), (1536, 8960, False, 0, False, True),
                                   (18944, 3584, True, 1, False, False), (3584, 18944, False, 0, False, True)])
def test_rows_gemv_fp8_frag_vs_bf16_frag(lib, shape, m_rows):
    """vv_linear on fp8 fragment-major codes + row scales against vv_linear on the bf16 fragment-major copy of the effective matrix code * scale:
    the same products summed in the same order, so the outputs must be IDENTICAL (ticketed split-K, deterministic) wherever both forms cut K
    alike (SPLIT_DIFFERS: to fp32 reassociation).  Whole-row, persistent dual SwiGLU, split-K ticket forms; then against fp64 torch at the bf16
    path's bar, and in place (res == out) with the atomic split-K form."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.weights import DeviceWeights
    n, k, dual, pro, mod, epi = shape
    m = m_rows
    L.check(lib.vv_tune(b"gemv_rows_scratch", 1), "scratch")
    try:
        torch.manual_seed(m * 1000 + n + k)
        x = torch.randn(m, k, device="cuda") * 1.5
        q1, s1, e1 = _quantised(n, k, n + k)
        q2, s2, e2 = _quantised(n, k, n + k + 1) if dual else (None, None, None)
        nw = torch.rand(k, device="cuda") + 0.5
        sh, sc = torch.randn(m, k, device="cuda") * 0.2, torch.randn(m, k, device="cuda") * 0.2
        gate, res, b = torch.randn(m, n, device="cuda"), torch.randn(m, n, device="cuda"), torch.randn(n, device="cuda")
        f8 = {1: DeviceWeights.frag_major_fp8(q1), 2: DeviceWeights.frag_major_fp8(q2) if dual else None}
        fb = {1: DeviceWeights.frag_major(e1), 2: DeviceWeights.frag_major(e2) if dual else None}
        assert f8[1] is not None and fb[1] is not None

        def args(fp8, out):
            a = L.LinArgs()
            a.x, a.ldx, a.m, a.n, a.k = x.data_ptr(), k, m, n, k
            a.flags = L.LIN_W_FRAG
            a.out, a.ldo = out.data_ptr(), n
            a.pro, a.eps = pro, 1e-5
            if pro == 1:
                a.norm_w = nw.data_ptr()
            if mod:
                a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
            f = f8 if fp8 else fb
            a.wdt = L.VV_FP8 if fp8 else L.VV_BF16
            a.w = f[1].data_ptr()
            if fp8:
                a.wscale = s1.data_ptr()
            if dual:
                a.w2, a.act = f[2].data_ptr(), 2
                if fp8:
                    a.w2scale = s2.data_ptr()
            if epi:
                a.gate, a.gate_ld, a.res, a.ldres = gate.data_ptr(), n, res.data_ptr(), n
            else:
                a.bias = b.data_ptr()
            return a

        lib.vv_tune(b"gemv_rows_atomic", 0)
        o8, o16 = torch.zeros(m, n, device="cuda"), torch.zeros(m, n, device="cuda")
        for _ in range(2):          # twice: the split-K tickets must be left ready for the next launch
            _run(lib, args(True, o8))
            _run(lib, args(False, o16))
        torch.cuda.synchronize()
        assert torch.isfinite(o8).all()
        if (n, k) in SPLIT_DIFFERS:
            e = rel_rms(o8.double().cpu().numpy(), o16.double().cpu().numpy())
            assert e < 1e-6, f"fp8-frag vs bf16-frag m={m} n={n} k={k} dual={dual} (other K slices): rel RMS {e:.3e}"
        else:
            nd = int((o8 != o16).sum())
            assert nd == 0, f"fp8-frag vs bf16-frag m={m} n={n} k={k} dual={dual}: {nd} outputs differ (max {(o8 - o16).abs().max().item():.3e})"
        # against fp64 torch on the effective matrices
        xd = x.double()
        if pro == 1:
            xd = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-5) * nw.double()
            if mod:
                xd = xd * (1 + sc.double()) + sh.double()
        y = xd @ e1.double().T
        if not epi:
            y = y + b.double()
        if dual:
            y = torch.nn.functional.silu(y) * (xd @ e2.double().T)
        if epi:
            y = y * gate.double() + res.double()
        err = rel_rms(o8.double().cpu().numpy(), y.cpu().numpy(), what=f"rows GEMV fp8 fragment-major m={m} n={n} k={k} dual={dual} vs fp64 torch")
        assert err < 2e-5, f"fp8 rows GEMV m={m} n={n} k={k} dual={dual}: rel RMS {err:.3e}"
        if epi:
            lib.vv_tune(b"gemv_rows_atomic", 1)
            out2 = res.clone()
            a = args(True, out2)
            a.res = out2.data_ptr()
            _run(lib, a)
            torch.cuda.synchronize()
            err = rel_rms(out2.double().cpu().numpy(), y.cpu().numpy())
            assert err < 2e-5, f"fp8 rows GEMV in place (atomic) m={m} n={n} k={k}: rel RMS {err:.3e}"
    finally:
        lib.vv_tune(b"gemv_rows_atomic", 1)
        lib.vv_tune(b"gemv_rows_scratch", 0)


def test_fp8_frag_flag_is_rejected_where_nothing_reads_that_layout(lib):
    """fp8 + VV_LIN_W_FRAG on a call the fp8 form of the matrix-core GEMV does not take is an error naming FRAG: 2 rows, k % 64 != 0, no row
    scale, and a long K with no split-K scratch."""
    from vibevoice_rocm_amd import _lib as L
    x = torch.randn(8, 8960, device="cuda")
    codes = torch.randint(0, 0x70, (1536, 8960), dtype=torch.uint8, device="cuda")
    scale = torch.full((1536,), 2.0 ** -8, device="cuda")
    out = torch.zeros(8, 1536, device="cuda")

    def args(m, k, with_scale=True):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt = x.data_ptr(), 8960, m, 1536, k, L.VV_FP8
        a.w, a.flags, a.out, a.ldo = codes.data_ptr(), L.LIN_W_FRAG, out.data_ptr(), 1536
        if with_scale:
            a.wscale = scale.data_ptr()
        return a

    s = torch.cuda.current_stream().cuda_stream
    for what, a in (("2 rows", args(2, 1536)), ("k % 64 != 0", args(8, 1568)), ("null wscale", args(8, 1536, False)),
                    ("long K, no split-K scratch", args(8, 8960))):
        assert lib.vv_linear(C.byref(a), s) != 0, what
        assert b"FRAG" in lib.vv_last_error(), (what, lib.vv_last_error())
    torch.cuda.synchronize()


def _fp8_frag_ptrs(w):
    """every f_* pointer of the LLM and head layers; asserts that each points at a uint8 (fp8 codes) fragment copy when the layer has fp8 companions"""
    by_ptr = {t.data_ptr(): t for t in w._frag_state["tensors"]}
    ptrs = []
    layers = [(w.llm.layer[l], ("qkv", "o", "gate", "up", "down")) for l in range(w.cfg.layers)]
    layers += [(w.head.layer[l], ("gate", "up", "down")) for l in range(w.cfg.head_layers)]
    for lay, names in layers:
        for nm in names:
            p = getattr(lay, "f_" + nm)
            assert p, f"f_{nm} missing"
            want = torch.uint8 if getattr(lay, "q_" + nm).q else torch.bfloat16
            assert by_ptr[p].dtype == want, f"f_{nm}: {by_ptr[p].dtype}"
            ptrs.append(p)
    return ptrs


def test_decode_step_8_rows_fp8_vs_batch2(big8):
    """One row-batched fp8 decode step (8 rows on the fp8 fragment-major codes) against the fp8 batch-2 step (1..2-row streaming fp8 GEMV) of
    every dialogue on its own engine state: hidden rows, constrained logits, tokens, positions."""
    from vibevoice_rocm_amd.rowbatch import RowBatch
    cfg, sd, m = big8
    tok = _Tok(cfg.vocab)
    ST, SD = tok.speech_start_id, tok.speech_diffusion_id
    valid = [ST, tok.speech_end_id, SD, tok.eos_token_id]
    B = 4
    lanes = [m._lane(b) for b in range(B)]
    rb = RowBatch(lanes)
    _fp8_frag_ptrs(m.engine.w)
    g = torch.Generator().manual_seed(17)
    lens = [50, 37, 44, 29]
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([ST])]) for n in lens]
    rb.begin(128, valid, 2.0)
    ref_h, ref_tok, ref_logits, ref_lens = [], [], [], []
    eng = m.engine
    for b in range(B):
        eng.begin_sequence(128, valid)
        x0 = eng.embed_ids(prompts[b])
        eng.prefill(x0, row=0, pos0=0)
        t0 = eng.first_token(ST, SD, SD)
        eng.prefill(eng.embed_ids(torch.tensor([ST])), row=1, pos0=0)
        with torch.cuda.stream(eng.stream):
            xin = torch.randn(cfg.hidden, generator=g).cuda() * 0.5
            eng.x2[0].copy_(xin); eng.x2[1].copy_(xin)
        t1 = eng.step_decode(ST, SD, None)
        eng.stream.synchronize()
        ref_h.append(eng.hidden2.clone()); ref_tok.append(t1); ref_logits.append(eng.logits[:4].clone()); ref_lens.append(eng.lens.clone())
        rb.prefill(b, x0)
        assert rb.first_token(b, SD) == t0 == SD
        rb.prefill(b, eng.embed_ids(torch.tensor([ST])), neg=True)
        with torch.cuda.stream(rb.stream):
            rb.x[2 * b].copy_(xin); rb.x[2 * b + 1].copy_(xin)
    rb.decode_begin(ST, SD, {b: None for b in range(B)})
    toks = rb.decode_end()
    rb.synchronize()
    for b in range(B):
        eh = rel_rms(rb.hidden[2 * b: 2 * b + 2].cpu().numpy(), ref_h[b].cpu().numpy(),
                     what=f"row-batched fp8 decode step 1.5B, dialogue {b} of 4: hidden rows vs the fp8 batch-2 step")
        el = rel_rms(rb.logits[b, :4].cpu().numpy(), ref_logits[b].cpu().numpy())
        assert eh < 5e-3 and el < 5e-3, f"dialogue {b}: hidden {eh:.3e} logits {el:.3e}"
        assert toks[b] == ref_tok[b]
        assert rb.lens[2 * b: 2 * b + 2].tolist() == ref_lens[b].tolist()
    rb.close()


@pytest.mark.parametrize("solver", ["ode", "sde"])
def test_head_sample_batch_fp8_vs_single(big8, solver):
    """The batched head sampler (4 utterances, 8 rows per pass over the fp8 fragment-major codes) against the fp8 single-utterance sampler, under
    the ODE and the SDE solver."""
    cfg, sd, m = big8
    eng = m.engine
    lb = eng.lib
    eng.w.ensure_frag()
    _fp8_frag_ptrs(eng.w)
    ode = m.model.noise_scheduler
    if solver == "sde":
        m.model.noise_scheduler = ode.from_config(ode.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")
        m.set_ddpm_inference_steps(N_STEPS)
        assert eng.sde
    try:
        B = 4
        g = torch.Generator().manual_seed(11 if solver == "ode" else 12)
        cond = torch.randn(2 * B, cfg.hidden, generator=g).cuda()
        noise = torch.randn(B, cfg.latent, generator=g).cuda()
        sde_noise = torch.randn(B, N_STEPS, cfg.latent, generator=g).cuda() if solver == "sde" else None
        with torch.cuda.stream(eng.stream):
            lat = torch.zeros(B, cfg.latent, device="cuda")
            if solver == "sde":
                ws = torch.empty(lb.vv_head_ws_bytes_batch_sde(C.byref(eng.w.head), N_STEPS, B), dtype=torch.uint8, device="cuda")
                eng._ck(lb.vv_head_sample_batch_sde(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(),
                                                    eng._coefs, N_STEPS, 2.0, lat.data_ptr(), cfg.latent, B, ws.data_ptr(), sde_noise.data_ptr(),
                                                    N_STEPS * cfg.latent, eng.sp), "vv_head_sample_batch_sde")
            else:
                ws = torch.empty(lb.vv_head_ws_bytes_batch(C.byref(eng.w.head), N_STEPS, B), dtype=torch.uint8, device="cuda")
                eng._ck(lb.vv_head_sample_batch(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(),
                                                eng._coefs, N_STEPS, 2.0, lat.data_ptr(), cfg.latent, B, ws.data_ptr(), eng.sp), "vv_head_sample_batch")
            one = torch.zeros(B, cfg.latent, device="cuda")
            for b in range(B):
                eng._ck(lb.vv_head_sample(C.byref(eng.w.head), cond[2 * b:].data_ptr(), cfg.hidden, noise[b].data_ptr(), eng.temb.data_ptr(), eng._coefs,
                                          N_STEPS, 2.0, one[b].data_ptr(), eng._head_ws.data_ptr(),
                                          None if sde_noise is None else sde_noise[b].data_ptr(), eng.sp), "vv_head_sample")
        eng.stream.synchronize()
        assert torch.isfinite(lat).all()
        for b in range(B):
            err = rel_rms(lat[b].cpu().numpy(), one[b].cpu().numpy(),
                          what=f"row-batched fp8 head sampling ({solver}) 1.5B, utterance {b} of 4, vs the fp8 single-utterance sampler")
            assert err < 2e-3, f"{solver} utterance {b}: rel RMS {err:.3e}"
    finally:
        m.model.noise_scheduler = ode
        m.set_ddpm_inference_steps(N_STEPS)


def _padded(tok, lens, g):
    S = tok.speech_start_id
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([S])]) for n in lens]
    Lp = max(lens)
    ids = torch.stack([torch.cat([torch.full((Lp - n,), tok.pad_id), p]) for n, p in zip(lens, prompts)])
    mask = torch.stack([torch.cat([torch.zeros(Lp - n, dtype=torch.long), torch.ones(n, dtype=torch.long)]) for n in lens])
    return ids, mask


def test_generate_fp8_takes_the_row_batched_path(big8):
    """generate() with weight_quant="fp8" on 4 dialogues runs the row-batched path; row_batch=False keeps the lanes."""
    cfg, sd, m = big8
    tok = _Tok(cfg.vocab)
    D, E, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id
    g = torch.Generator().manual_seed(5)
    ids, mask = _padded(tok, [30, 24, 28, 21], g)
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=[[D, D, E, EOS]] * 4,
              noise=torch.randn(4, 4, cfg.latent, generator=g))
    m.release_lanes()
    m.generate(row_batch=False, **kw)
    assert not m._rowbatch, "row_batch=False took the row-batched path"
    m.generate(**kw)
    assert (4, 0) in m._rowbatch, "weight_quant='fp8' on 4 dialogues did not take the row-batched path"


@pytest.mark.parametrize("B", [4, 9])
def test_generate_fp8_row_batch_vs_lanes(big8, B):
    """fp8 generate() row-batched (4 dialogues: one row batch; 9: three) against the fp8 lanes with different token schedules (an early end, a
    turn switch with rolled-back speculative frames): same sequences, waveforms to the rounding of the matrix-core GEMV."""
    cfg, sd, m = big8
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(61 + B)
    ids, mask = _padded(tok, [50 - 3 * (b % 5) for b in range(B)], g)
    forced = [[D] * (3 + (b % 4)) + ([E, S, D, D] if b % 3 == 1 else []) + [E, EOS] for b in range(B)]
    noise = torch.randn(B, 10, cfg.latent, generator=g)
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    m.release_lanes()
    lanes = m.generate(row_batch=False, **kw)
    rows = m.generate(row_batch=True, **kw)
    assert m._rowbatch, "the fp8 batch did not take the row-batched path"
    assert rows.sequences.tolist() == lanes.sequences.tolist()
    for b in range(B):
        a, r = rows.speech_outputs[b], lanes.speech_outputs[b]
        assert a.shape == r.shape
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what=f"generate() fp8 on {B} dialogues 1.5B, row-batched vs lanes, waveform of dialogue {b}")
        assert err < 1e-2, f"{B} dialogues, dialogue {b}: waveform rel RMS {err:.3e}"


def test_generate_fp8_sampling_sde_row_batch_reproducible(big8):
    """SDE solver + do_sample, nothing injected, fp8 row-batched: finite audio, constrained tokens, and the same seed gives the same sequences."""
    cfg, sd, m = big8
    tok = _Tok(cfg.vocab)
    valid = {tok.speech_start_id, tok.speech_end_id, tok.speech_diffusion_id, tok.eos_token_id}
    ode = m.model.noise_scheduler
    m.model.noise_scheduler = ode.from_config(ode.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")
    m.set_ddpm_inference_steps(N_STEPS)
    try:
        g = torch.Generator().manual_seed(47)
        ids, mask = _padded(tok, [30, 24, 28, 21], g)
        kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, max_new_tokens=12,
                  generation_config={"do_sample": True, "temperature": 1.0, "top_p": 0.95})
        outs = []
        m.release_lanes()
        for _ in range(2):
            torch.manual_seed(1234)
            outs.append(m.generate(row_batch=True, **kw))
        assert (4, 0) in m._rowbatch
        assert outs[0].sequences.tolist() == outs[1].sequences.tolist()
        Lp = ids.shape[1]
        for b, seq in enumerate(outs[0].sequences.tolist()):
            gen = seq[Lp:]
            n = len(gen) - next((i for i, t in enumerate(reversed(gen)) if t != tok.pad_id), len(gen))
            assert n > 0 and all(t in valid for t in gen[:n]), f"dialogue {b}: {gen}"
            a = outs[0].speech_outputs[b]
            if a is not None:
                assert torch.isfinite(a).all(), f"dialogue {b}: non-finite audio"
    finally:
        m.model.noise_scheduler = ode
        m.set_ddpm_inference_steps(N_STEPS)


def test_generate_fp8_row_batch_mid_vs_oracle():
    """fp8 row-batched generate() at `mid` shapes on 3 dialogues against the CPU oracle run on fp8_effective_state_dict (the matrices the fp8 codes
    stand for), at the bar of the single-dialogue fp8 test (2e-2); the fp8 lanes' error next to it in the parity record."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import vv_oracle as O
    from test_hip_configs import _four_speaker_inputs, _special
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict
    from vibevoice_rocm_amd.weights import fp8_effective_state_dict, fp8_matrix_names
    cfg = VVConfig.preset("mid")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 4321).items()}
    eff = fp8_effective_state_dict(cfg, sd)
    names = set(fp8_matrix_names(cfg))
    sd_o = {k: (eff[k] if k in names else (v.to(torch.bfloat16).float() if v.dim() >= 2 else v)) for k, v in sd.items()}
    V = cfg.vocab
    ST, SE, SD, EOS = V - 4, V - 3, V - 2, V - 1
    g = torch.Generator().manual_seed(29)
    ids, sp_mask, wav, sm = _four_speaker_inputs(cfg, g)
    forced = [([SD] * 4 + [SE, ST]) * 2 + [SD] * 4 + [SE, EOS], [SD] * 7 + [SE, ST] + [SD] * 3 + [SE, EOS], [SD] * 5 + [SE, EOS]]
    noise = torch.randn(3, 12, cfg.latent, generator=g)
    std_noise, eps_noise = torch.randn(4, generator=g), torch.randn(4, 4, cfg.ac_dim, generator=g)
    _, conn = O.process_speech_inputs(sd_o, cfg.as_dict(), wav, sm, std_noise, eps_noise)
    refs = [O.generate(sd_o, cfg.as_dict(), ids.tolist(), sp_mask, conn, _special(V), noise[b], cfg_scale=2.0, n_steps=20, forced_tokens=forced[b], bf16_t=True)
            for b in range(3)]
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="fp8")
    m.set_ddpm_inference_steps(20)
    tok = _Tok(V)
    tok.pad_id = 0
    kw = dict(input_ids=ids[None].repeat(3, 1), attention_mask=torch.ones(3, ids.shape[0], dtype=torch.long), speech_tensors=wav.repeat(3, 1), speech_masks=sm.repeat(3, 1),
              speech_input_mask=sp_mask[None].repeat(3, 1), tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise,
              speech_noise=(std_noise.repeat(3), eps_noise.repeat(3, 1, 1)))
    outs = {rbm: m.generate(row_batch=rbm, **kw) for rbm in (True, False)}
    assert (3, 0) in m._rowbatch
    _fp8_frag_ptrs(m.engine.w)
    for b in range(3):
        want = torch.cat(refs[b].audio).numpy()
        assert outs[True].sequences[b, ids.shape[0]: ids.shape[0] + len(forced[b])].tolist() == forced[b]
        e_rows = rel_rms(outs[True].speech_outputs[b][0].float().cpu().numpy(), want, what=f"generate() 3 dialogues, mid fp8, ROW-BATCHED vs oracle, dialogue {b}")
        e_lane = rel_rms(outs[False].speech_outputs[b][0].float().cpu().numpy(), want, what=f"generate() 3 dialogues, mid fp8, lanes vs oracle, dialogue {b}")
        assert e_rows < 2e-2, f"row-batched fp8 dialogue {b}: waveform rel RMS {e_rows:.3e} vs oracle (lanes: {e_lane:.3e})"


@pytest.mark.parametrize("quant", [None, "fp8"])
def test_fragment_copies_are_built_once_per_process(quant):
    """A 4-dialogue call, then an 8-dialogue call (two row batches, the second led by a forked lane): the fragment-major copies are built once
    for the weights and every fork - the f_* pointers stay, and asking any lane again allocates nothing."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset("mid")
    sd = synth_state_dict_torch(cfg, 99, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=quant)
    m.set_ddpm_inference_steps(10)
    tok = _Tok(cfg.vocab)
    D, E, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id
    g = torch.Generator().manual_seed(3)

    def call(B):
        ids, mask = _padded(tok, [20 + b for b in range(B)], g)
        m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=[[D, D, E, EOS]] * B,
                   noise=torch.randn(B, 4, cfg.latent, generator=g))

    call(4)
    assert (4, 0) in m._rowbatch
    w = m.engine.w
    ptrs = _fp8_frag_ptrs(w)
    n_frag = len(w._frag_state["tensors"])
    call(8)
    assert (4, 4, "side") in m._rowbatch
    torch.cuda.synchronize()
    assert _fp8_frag_ptrs(w) == ptrs and len(w._frag_state["tensors"]) == n_frag
    mem = torch.cuda.memory_allocated()
    for e in m._lanes:
        e.w.ensure_frag()
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == mem, "a forked lane built its own fragment copies"
    assert _fp8_frag_ptrs(w) == ptrs
    del m
    torch.cuda.empty_cache()
