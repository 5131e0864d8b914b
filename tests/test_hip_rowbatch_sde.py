"""GPU parity of the row-batched decode path under the SDE solver (sde-dpmsolver++, the scheduler main.py sets up) and with sampled tokens
(do_sample / temperature / top_p): vv_head_sample_batch_sde against the single-utterance sampler and the CPU oracle, its ODE form against
vv_head_sample_batch bit for bit, and generate() row-batched against the lanes - same sequences, same random draws (the CPU generator is left in
the same state), waveforms to the rounding of the matrix-core GEMV.  Measured errors go into the parity record (conftest.rel_rms `what=`)."""
import ctypes as C

import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

N_STEPS = 20
VV_E_UNSUPPORTED = -3          # include/vv_hip.h


def _sde_scheduler(sched):
    return sched.from_config(sched.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")


@pytest.fixture(scope="module")
def big():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset("1.5b")
    sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m.set_ddpm_inference_steps(N_STEPS)
    return cfg, sd, m


@pytest.fixture
def sde(big):
    """the module's model with the SDE scheduler swapped in as main.py does it (model.model.noise_scheduler = ...from_config), ODE restored after"""
    cfg, sd, m = big
    ode = m.model.noise_scheduler
    m.model.noise_scheduler = _sde_scheduler(ode)
    m.set_ddpm_inference_steps(N_STEPS)
    assert m.engine.sde and m.engine._coefs[0].cn > 0
    try:
        yield cfg, sd, m
    finally:
        m.model.noise_scheduler = ode
        m.set_ddpm_inference_steps(N_STEPS)


class _Tok:
    def __init__(self, vocab):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = vocab - 4, vocab - 3, vocab - 2, vocab - 1
        self.bos_token_id = None
        self.pad_id = vocab - 5


def _sample_batch_sde(eng, cond, noise, sde_noise, B, cfg_scale):
    """vv_head_sample_batch_sde on the engine's schedule; sde_noise [B, n_steps, latent] or None"""
    cfg = eng.cfg
    lb = eng.lib
    with torch.cuda.stream(eng.stream):
        ws = torch.empty(lb.vv_head_ws_bytes_batch_sde(C.byref(eng.w.head), eng.n_steps, B), dtype=torch.uint8, device="cuda")
        lat = torch.zeros(B, cfg.latent, device="cuda")
        rc = lb.vv_head_sample_batch_sde(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(), eng._coefs,
                                         eng.n_steps, cfg_scale, lat.data_ptr(), cfg.latent, B, ws.data_ptr(),
                                         None if sde_noise is None else sde_noise.data_ptr(), eng.n_steps * cfg.latent, eng.sp)
    eng._ck(rc, "vv_head_sample_batch_sde")
    eng.stream.synchronize()
    return lat


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_head_sample_batch_sde_vs_single(sde, B):
    """Under the SDE solver: the batched sampler (variance noise mapped into the fused boundary's state space, one launch for all steps and
    utterances) against vv_head_sample per utterance (the three-launch boundary) with the same [n_steps, latent] noise of each utterance."""
    cfg, sd, m = sde
    eng = m.engine
    eng.w.ensure_frag()
    g = torch.Generator().manual_seed(100 + B)
    cond = torch.randn(2 * B, cfg.hidden, generator=g).cuda()
    noise = torch.randn(B, cfg.latent, generator=g).cuda()
    sde_noise = torch.randn(B, N_STEPS, cfg.latent, generator=g).cuda()
    lat = _sample_batch_sde(eng, cond, noise, sde_noise, B, 2.0)
    one = torch.zeros(B, cfg.latent, device="cuda")
    with torch.cuda.stream(eng.stream):
        for b in range(B):
            eng._ck(eng.lib.vv_head_sample(C.byref(eng.w.head), cond[2 * b:].data_ptr(), cfg.hidden, noise[b].data_ptr(), eng.temb.data_ptr(), eng._coefs,
                                           N_STEPS, 2.0, one[b].data_ptr(), eng._head_ws.data_ptr(), sde_noise[b].data_ptr(), eng.sp), "vv_head_sample")
    eng.stream.synchronize()
    # the noise is applied: the same utterances with zero variance noise land elsewhere
    assert not torch.allclose(lat, _sample_batch_sde(eng, cond, noise, torch.zeros_like(sde_noise), B, 2.0), rtol=1e-2, atol=1e-2)
    for b in range(B):
        err = rel_rms(lat[b].cpu().numpy(), one[b].cpu().numpy(), what=f"row-batched SDE head sampling 1.5B, utterance {b} of {B}, vs the single-utterance sampler")
        assert err < 2e-3, f"B={B} utterance {b}: rel RMS {err:.3e}"


def test_head_sample_batch_sde_ode_form_is_identical(big):
    """With sde_noise = NULL under the ODE scheduler the new entry point launches exactly what vv_head_sample_batch launches: bit-identical.
    vv_head_sample_batch keeps refusing SDE coefficients (VV_E_UNSUPPORTED), and the SDE form refuses them without noise."""
    from vibevoice_rocm_amd import _lib as L
    cfg, sd, m = big
    eng = m.engine
    assert not eng.sde
    eng.w.ensure_frag()
    lb = eng.lib
    B = 4
    g = torch.Generator().manual_seed(12)
    cond = torch.randn(2 * B, cfg.hidden, generator=g).cuda()
    noise = torch.randn(B, cfg.latent, generator=g).cuda()
    ws = torch.empty(lb.vv_head_ws_bytes_batch(C.byref(eng.w.head), N_STEPS, B), dtype=torch.uint8, device="cuda")
    want = torch.zeros(B, cfg.latent, device="cuda")
    # the head's down projection folds its K slices with fp32 atomics by default (summation order varies run to run): bit for bit needs the
    # deterministic ticket form of the rows GEMV
    L.check(lb.vv_tune(b"gemv_rows_atomic", 0), "gemv_rows_atomic")
    try:
        got = _sample_batch_sde(eng, cond, noise, None, B, 2.0)
        with torch.cuda.stream(eng.stream):
            eng._ck(lb.vv_head_sample_batch(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(), eng._coefs,
                                            N_STEPS, 2.0, want.data_ptr(), cfg.latent, B, ws.data_ptr(), eng.sp), "vv_head_sample_batch")
        eng.stream.synchronize()
    finally:
        lb.vv_tune(b"gemv_rows_atomic", 1)
    assert torch.equal(got, want)
    assert lb.vv_head_ws_bytes_batch_sde(C.byref(eng.w.head), N_STEPS, B) > lb.vv_head_ws_bytes_batch(C.byref(eng.w.head), N_STEPS, B)
    # SDE coefficients: refused by the ODE-only entry point, and by the SDE one without noise
    sched = _sde_scheduler(eng.scheduler)
    sched.set_timesteps(N_STEPS)
    coefs = (L.DpmCoef * N_STEPS)()
    for i, c in enumerate(sched.coefs):
        coefs[i].alpha_s, coefs[i].sigma_s, coefs[i].cx, coefs[i].cd = c["alpha_s"], c["sigma_s"], c["cx"], c["cd"]
        coefs[i].rinv, coefs[i].order, coefs[i].cn = c["rinv"], c["order"], c["cn"]
    assert coefs[0].cn > 0
    with torch.cuda.stream(eng.stream):
        rc = lb.vv_head_sample_batch(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(), coefs, N_STEPS,
                                     2.0, want.data_ptr(), cfg.latent, B, ws.data_ptr(), eng.sp)
        assert rc == VV_E_UNSUPPORTED, rc
        ws2 = torch.empty(lb.vv_head_ws_bytes_batch_sde(C.byref(eng.w.head), N_STEPS, B), dtype=torch.uint8, device="cuda")
        rc = lb.vv_head_sample_batch_sde(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(), coefs, N_STEPS,
                                         2.0, want.data_ptr(), cfg.latent, B, ws2.data_ptr(), None, N_STEPS * cfg.latent, eng.sp)
        assert rc != 0
    eng.stream.synchronize()


def test_head_sample_batch_sde_mid_vs_oracle():
    """The batched SDE sampler at `mid` shapes (bf16 weights), 3 utterances in one call, each against the CPU oracle's sde-dpmsolver++ loop with
    the same initial and variance noise, at the bar of the single-utterance SDE test (test_generate_with_sde_solver_mid_vs_oracle)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("mid")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 4321).items()}
    sd_o = {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 else v) for k, v in sd.items()}
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m.model.noise_scheduler = _sde_scheduler(m.model.noise_scheduler)
    m.set_ddpm_inference_steps(num_steps=10)
    eng = m.engine
    assert eng.sde
    eng.w.ensure_frag()
    B = 3
    g = torch.Generator().manual_seed(23)
    cond = torch.randn(2 * B, cfg.hidden, generator=g)
    noise = torch.randn(B, cfg.latent, generator=g)
    sde_noise = torch.randn(B, 10, cfg.latent, generator=g)
    lat = _sample_batch_sde(eng, cond.cuda(), noise.cuda(), sde_noise.cuda(), B, 1.5)
    for b in range(B):
        want = O.sample_speech_tokens(sd_o, cfg.as_dict(), cond[2 * b: 2 * b + 1], cond[2 * b + 1: 2 * b + 2], noise[b: b + 1], 1.5, 10,
                                      algorithm="sde-dpmsolver++", sde_noise=sde_noise[b][:, None], bf16_t=True)
        err = rel_rms(lat[b].cpu().numpy(), want[0].numpy(), what=f"row-batched SDE head sampling mid bf16, utterance {b} of 3, vs oracle")
        assert err < 2e-2, f"utterance {b}: SDE sampling bf16 vs oracle: rel RMS {err:.3e}"


def _padded(cfg, tok, lens, g):
    S = tok.speech_start_id
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([S])]) for n in lens]
    Lp = max(lens)
    ids = torch.stack([torch.cat([torch.full((Lp - n,), tok.pad_id), p]) for n, p in zip(lens, prompts)])
    mask = torch.stack([torch.cat([torch.zeros(Lp - n, dtype=torch.long), torch.ones(n, dtype=torch.long)]) for n in lens])
    return ids, mask


def _run_both(m, B, **kw):
    """lanes, then the row-batched call on freshly created row batches (release_lanes: no earlier call can have made the keys); chunk events of both"""
    from vibevoice_rocm_amd.streamer import AudioStreamer
    outs, events = {}, {}
    for rbm in (False, True):
        if rbm:
            m.release_lanes()
        st = AudioStreamer(batch_size=B)
        ev = []
        put0 = st.put

        def spy(chunks, idx, put0=put0, ev=ev):
            ev.append([int(i) for i in idx])
            put0(chunks, idx)
        st.put = spy
        outs[rbm] = m.generate(audio_streamer=st, row_batch=rbm, **kw)
        events[rbm] = ev
        if rbm:
            for b in range(B):
                got = [c.reshape(-1) for c in st.get_stream(b)]
                if outs[rbm].speech_outputs[b] is not None:
                    assert torch.equal(torch.cat(got), outs[rbm].speech_outputs[b][0].cpu()), f"sample {b}: streamed chunks"
    return outs, events


def _compare_audio(outs, B, what, bar=1e-2):
    for b in range(B):
        a, r = outs[True].speech_outputs[b], outs[False].speech_outputs[b]
        assert (a is None) == (r is None), f"dialogue {b}: audio on one path only"
        if a is None:
            continue
        assert a.shape == r.shape
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what=f"{what}, waveform of dialogue {b}")
        assert err < bar, f"{what}, dialogue {b}: waveform rel RMS {err:.3e}"


def test_generate_sde_row_batch_vs_lanes(sde):
    """generate() on 4 left-padded dialogues under the SDE solver with injected initial and variance noise, mixed schedules (an early EOS, a turn
    switch: mis-speculated frames roll back): the row-batched path is taken and agrees with the lanes - same sequences, same chunk delivery,
    waveforms to the rounding of the matrix-core GEMV.  Then 6 dialogues (two row batches of 3)."""
    cfg, sd, m = sde
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(31)
    ids, mask = _padded(cfg, tok, [50, 37, 44, 29], g)
    forced = [[D] * 6 + [E, EOS], [D] * 2 + [E, EOS], [D] * 3 + [E, S] + [D] * 2 + [E, EOS], [D] * 5 + [E, EOS]]
    noise = torch.randn(4, 8, cfg.latent, generator=g)
    sde_noise = torch.randn(4, 8, N_STEPS, cfg.latent, generator=g)
    outs, events = _run_both(m, 4, input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise, sde_noise=sde_noise)
    assert (4, 0) in m._rowbatch, "the SDE batch did not take the row-batched path"
    assert outs[True].sequences.tolist() == outs[False].sequences.tolist()
    assert events[True] == events[False]
    _compare_audio(outs, 4, "generate() SDE on 4 dialogues 1.5B bf16, row-batched vs lanes")
    # six dialogues: two row batches of 3, every conv tail beside the main stream
    B = 6
    ids6, mask6 = _padded(cfg, tok, [40, 33, 40, 27, 38, 40], g)
    forced6 = [[D] * (3 + (b % 3)) + ([E, S, D, D] if b == 1 else []) + [E, EOS] for b in range(B)]
    noise6 = torch.randn(B, 8, cfg.latent, generator=g)
    sde6 = torch.randn(B, 8, N_STEPS, cfg.latent, generator=g)
    outs, events = _run_both(m, B, input_ids=ids6, attention_mask=mask6, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced6, noise=noise6, sde_noise=sde6)
    assert (3, 0, "side") in m._rowbatch and (3, 3, "side") in m._rowbatch
    assert outs[True].sequences.tolist() == outs[False].sequences.tolist()
    assert events[True] == events[False]
    _compare_audio(outs, B, "generate() SDE on 6 dialogues (two row batches) 1.5B bf16, row-batched vs lanes")


def test_generate_sampling_sde_row_batch_vs_lanes(sde):
    """generate() on 4 dialogues as the reference's application calls it: SDE solver, do_sample with temperature / top_p, nothing injected (every
    token and every noise row is drawn from torch's CPU generator).  Seeded alike, the row-batched call draws the same tokens as the lanes and
    leaves the generator in the same state (same draws in the same order); waveforms agree; every token is in the constrained set."""
    cfg, sd, m = sde
    tok = _Tok(cfg.vocab)
    valid = {tok.speech_start_id, tok.speech_end_id, tok.speech_diffusion_id, tok.eos_token_id}
    g = torch.Generator().manual_seed(47)
    ids, mask = _padded(cfg, tok, [30, 24, 28, 21], g)
    Lp = ids.shape[1]
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, max_new_tokens=12,
              generation_config={"do_sample": True, "temperature": 1.0, "top_p": 0.95})
    outs, rng = {}, {}
    for rbm in (False, True):
        if rbm:
            m.release_lanes()
        torch.manual_seed(1234)
        outs[rbm] = m.generate(row_batch=rbm, **kw)
        rng[rbm] = torch.get_rng_state()
    assert (4, 0) in m._rowbatch, "the sampled SDE batch did not take the row-batched path"
    seqs = outs[True].sequences.tolist()
    assert seqs == outs[False].sequences.tolist()
    assert torch.equal(rng[True], rng[False]), "the row-batched call drew a different amount / order of random numbers"
    for b in range(4):
        gen = seqs[b][Lp:]
        n = len(gen) - next((i for i, t in enumerate(reversed(gen)) if t != tok.pad_id), len(gen))
        assert n > 0 and all(t in valid for t in gen[:n]) and all(t == tok.pad_id for t in gen[n:]), f"dialogue {b}: {gen}"
    assert sum(o is not None for o in outs[True].speech_outputs) >= 2, "the seed gave too little speech to compare"
    _compare_audio(outs, 4, "generate() sampled tokens + SDE on 4 dialogues 1.5B bf16, row-batched vs lanes")
