"""GPU tests of serving sessions (model.open_session): vv_head_sample_batch_cfg - the batched diffusion sampler with one guidance scale per
utterance, read on the device - against the scalar entry points; a session that refills its slots mid-flight against generate() on every
dialogue alone; device noise, device-side sampling, generate(cfg_scale=[...]) and the untouched default path.  Shapes and bars are those of
the row-batch suite (tests/test_hip_rowbatch.py); the measured errors go into the parity record (conftest.rel_rms `what=`)."""
import ctypes as C
import math

import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

N_STEPS = 20
VV_E_ARG = -1                  # include/vv_hip.h


def _sde_scheduler(sched):
    return sched.from_config(sched.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")


def _model(preset, seed):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset(preset)
    sd = synth_state_dict_torch(cfg, seed, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m.set_ddpm_inference_steps(N_STEPS)
    return cfg, m


@pytest.fixture(scope="module")
def big():
    return _model("1.5b", 2024)


@pytest.fixture(scope="module")
def mid():
    return _model("mid", 4321)


class _Solver:
    """the model with the SDE scheduler swapped in as the reference's callers do it, the ODE one restored on exit"""

    def __init__(self, m, sde):
        self.m, self.sde = m, sde

    def __enter__(self):
        if self.sde:
            self.ode = self.m.model.noise_scheduler
            self.m.model.noise_scheduler = _sde_scheduler(self.ode)
            self.m.set_ddpm_inference_steps(N_STEPS)
            assert self.m.engine.sde and self.m.engine._coefs[0].cn > 0

    def __exit__(self, *exc):
        if self.sde:
            self.m.model.noise_scheduler = self.ode
            self.m.set_ddpm_inference_steps(N_STEPS)
        return False


class _Tok:
    def __init__(self, vocab):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = vocab - 4, vocab - 3, vocab - 2, vocab - 1
        self.bos_token_id = None
        self.pad_id = vocab - 5


# ---- 1. guidance per utterance ----------------------------------------------------------------------------------------------------
def _head_scalar(eng, cond, noise, sde_noise, B, scale):
    cfg, lb = eng.cfg, eng.lib
    with torch.cuda.stream(eng.stream):
        lat = torch.zeros(B, cfg.latent, device="cuda")
        if sde_noise is not None:
            ws = torch.empty(lb.vv_head_ws_bytes_batch_sde(C.byref(eng.w.head), eng.n_steps, B), dtype=torch.uint8, device="cuda")
            rc = lb.vv_head_sample_batch_sde(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(), eng._coefs,
                                             eng.n_steps, scale, lat.data_ptr(), cfg.latent, B, ws.data_ptr(), sde_noise.data_ptr(), eng.n_steps * cfg.latent, eng.sp)
        else:
            ws = torch.empty(lb.vv_head_ws_bytes_batch(C.byref(eng.w.head), eng.n_steps, B), dtype=torch.uint8, device="cuda")
            rc = lb.vv_head_sample_batch(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(), eng._coefs,
                                         eng.n_steps, scale, lat.data_ptr(), cfg.latent, B, ws.data_ptr(), eng.sp)
    eng._ck(rc, "scalar sampler")
    eng.stream.synchronize()
    return lat


def _head_rows(eng, cond, noise, sde_noise, B, scales, check=True):
    cfg, lb = eng.cfg, eng.lib
    with torch.cuda.stream(eng.stream):
        lat = torch.zeros(B, cfg.latent, device="cuda")
        rows = None if scales is None else torch.tensor(scales, dtype=torch.float32, device="cuda")
        nb = (lb.vv_head_ws_bytes_batch_sde if sde_noise is not None else lb.vv_head_ws_bytes_batch)(C.byref(eng.w.head), eng.n_steps, B)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        rc = lb.vv_head_sample_batch_cfg(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(), eng._coefs,
                                         eng.n_steps, None if rows is None else rows.data_ptr(), lat.data_ptr(), cfg.latent, B, ws.data_ptr(),
                                         None if sde_noise is None else sde_noise.data_ptr(), eng.n_steps * cfg.latent if sde_noise is not None else 0, eng.sp)
    if not check:
        return rc
    eng._ck(rc, "vv_head_sample_batch_cfg")
    eng.stream.synchronize()
    return lat


@pytest.mark.parametrize("sde", [False, True], ids=["ode", "sde"])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("preset", ["mid", "1.5b"])
def test_head_sample_batch_cfg_vs_scalar(request, preset, B, sde):
    """vv_head_sample_batch_cfg with cfg_rows = (1.0, 1.3, 3.0[, 2.0]) on the heads of the `mid` (D = 512) and 1.5B (D = 1536) presets - two
    KU instantiations of the boundary kernel - ODE and SDE: utterance b agrees with the scalar entry point at cfg_b on the same inputs to the
    bar of test_head_sample_batch_vs_single (2e-3; the split-K accumulation order is the only difference: measured 0 at `mid`, <= 7.3e-7 at 1.5B),
    while the scalar entry at
    its NEIGHBOUR's scale puts utterance b more than 10 x the bar away (measured 0.15 .. 1.3) - a sampler that read one scale for all, or another utterance's, would
    be caught.  A uniform cfg_rows agrees with the scalar call; a null cfg_rows is VV_E_ARG.  The 7B head (D = 3584) is not run: its
    construction needs the whole 7B model (test_generate_row_batch_7b_shapes_vs_lanes), too much for a test of a few seconds."""
    cfg, m = request.getfixturevalue("mid" if preset == "mid" else "big")
    eng = m.engine
    with _Solver(m, sde):
        eng.w.ensure_frag()
        g = torch.Generator().manual_seed(300 + 10 * B + sde)
        cond = torch.randn(2 * B, cfg.hidden, generator=g).cuda()
        noise = torch.randn(B, cfg.latent, generator=g).cuda()
        sde_noise = torch.randn(B, N_STEPS, cfg.latent, generator=g).cuda() if sde else None
        scales = [1.0, 1.3, 3.0, 2.0][:B]
        got = _head_rows(eng, cond, noise, sde_noise, B, scales)
        scalar = {c: _head_scalar(eng, cond, noise, sde_noise, B, c) for c in scales}
        tag = f"{preset} head, {'SDE' if sde else 'ODE'}, utterance %d of {B}"
        for b in range(B):
            own, other = scalar[scales[b]][b].cpu().numpy(), scalar[scales[(b + 1) % B]][b].cpu().numpy()
            err = rel_rms(got[b].cpu().numpy(), own, what=f"vv_head_sample_batch_cfg vs the scalar entry at its own scale {scales[b]}: " + tag % b)
            far = rel_rms(other, own, what=f"scalar entry at the neighbour's scale {scales[(b + 1) % B]} vs at its own {scales[b]}: " + tag % b)
            print(f"{tag % b}: own {err:.3e}, neighbour's scale {far:.3e}")
            assert err < 2e-3, f"utterance {b}: rel RMS {err:.3e}"
            assert far > 2e-2, f"utterance {b}: the neighbour's scale moves the sample by only {far:.3e}: the comparison would not tell them apart"
        uni = _head_rows(eng, cond, noise, sde_noise, B, [2.0] * B)
        want = scalar[2.0] if 2.0 in scalar else _head_scalar(eng, cond, noise, sde_noise, B, 2.0)
        for b in range(B):
            err = rel_rms(uni[b].cpu().numpy(), want[b].cpu().numpy(), what="uniform cfg_rows 2.0 vs the scalar entry: " + tag % b)
            assert err < 2e-3, f"uniform, utterance {b}: rel RMS {err:.3e}"
        assert _head_rows(eng, cond, noise, sde_noise, B, None, check=False) == VV_E_ARG
        assert b"cfg_rows" in eng.lib.vv_last_error()
        eng.stream.synchronize()


# ---- 2. a session against every dialogue alone ------------------------------------------------------------------------------------
LENS = [50, 48, 44, 37, 29, 33, 41, 30, 36]
SCALES = [1.3, 2.0, 3.0, 2.0, 1.3, 3.0, 1.3, 2.0, 3.0]
STREAMED = 2


def _workload(cfg):
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(61)
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([S])]) for n in LENS]
    forced = [[D] * 8 + [E, EOS], [D] * 2 + [E, EOS],                      # 1 ends early: its slot goes to a dialogue with a shorter context
              [D] * 3 + [E, S] + [D] * 2 + [E, EOS],                       # 2 switches turns (a speculated frame rolled back), and is streamed
              [D] * 5 + [E, EOS], [D] * 4 + [E, EOS], [D] * 6 + [E, EOS], [D] * 2 + [E, EOS], [D] * 3 + [E, EOS],
              [D] * 4 + [E, S] + [D] * 2 + [E, EOS]]
    noise = torch.randn(len(LENS), 8, cfg.latent, generator=g)
    return tok, prompts, forced, noise


_ALONE = {}


def _alone(big):
    """generate() on every dialogue of the workload alone (computed once, after the sessions have closed; never changed)"""
    if not _ALONE:
        cfg, m = big
        tok, prompts, forced, noise = _workload(cfg)
        for i in range(len(LENS)):
            _ALONE[i] = m.generate(input_ids=prompts[i][None], tokenizer=tok, cfg_scale=SCALES[i], forced_tokens=forced[i], noise=noise[i])
    return _ALONE


@pytest.mark.parametrize("slots", [4, 6])
def test_session_vs_each_dialogue_alone(big, slots):
    """Nine dialogues - prompts of 29..50 tokens, 2..8 frames, two turn switches, early ends, injected noise, guidance 1.3 / 2.0 / 3.0 mixed
    within a row batch - through a session of 4 slots (one row batch) and of 6 (two): five submitted at once, the rest after three steps, so a
    queue forms and slots are refilled mid-flight.  Every dialogue against generate() on it alone (the single-dialogue engine, run after
    close()): same sequence, waveform to the row-batched-vs-lanes bar at these shapes (1e-2); the streamed chunks are the returned audio bit for
    bit; and a slot was reused by a dialogue with a SHORTER context than its previous occupant (stale K / V / vt beyond the new positions)."""
    from vibevoice_rocm_amd.streamer import AudioStreamer
    cfg, m = big
    tok, prompts, forced, noise = _workload(cfg)
    st = AudioStreamer(batch_size=1)
    sess = m.open_session(tokenizer=tok, slots=slots, max_context=256, device_noise=False)
    with pytest.raises(RuntimeError):
        m.generate(input_ids=prompts[0][None], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[0], noise=noise[0])
    with pytest.raises(RuntimeError):
        m.open_session(tokenizer=tok, slots=2, max_context=256)

    def submit(i):
        return sess.submit(input_ids=prompts[i][None], cfg_scale=SCALES[i], forced_tokens=forced[i], noise=noise[i],
                           audio_streamer=st if i == STREAMED else None)
    hs = {i: submit(i) for i in range(5)}
    for _ in range(3):
        assert sess.step()
    assert sum(h.slot is None for h in hs.values()) == max(0, 5 - slots) and [i for i, h in hs.items() if h.done] == [1]      # 1 has just ended
    hs.update({i: submit(i) for i in range(5, len(LENS))})
    sess.run()
    sess.close()
    assert m._session is None and all(h.done for h in hs.values())
    assert all(k in m._rowbatch for k in ([(4, 0, "session")] if slots == 4 else [(3, 0, "session", "side"), (3, 3, "session", "side")]))
    for rb, _ in sess.driver.groups:
        assert rb._graphs and all(not any(isinstance(x, float) for x in key) for key in rb._graphs), list(rb._graphs)      # no scale in any graph key
    streamed = torch.cat([c.reshape(-1) for c in st.get_stream(0)])
    assert torch.equal(streamed, hs[STREAMED].result().speech_outputs[0][0].cpu()) and st.finished_flags == [True]
    by_slot = {}
    for i in range(len(LENS)):                                       # admission is FIFO: submission order is occupation order
        by_slot.setdefault(hs[i].slot, []).append(LENS[i] + len(forced[i]))
    assert set(by_slot) <= set(range(slots)) and sum(len(v) for v in by_slot.values()) == len(LENS)
    assert any(b < a for v in by_slot.values() for a, b in zip(v, v[1:])), by_slot
    alone = _alone(big)
    for i in range(len(LENS)):
        got, want = hs[i].result(), alone[i]
        assert got.sequences.tolist() == want.sequences.tolist() == [prompts[i].tolist() + forced[i]], i
        a, r = got.speech_outputs[0], want.speech_outputs[0]
        assert a.shape == r.shape and not got.reach_max_step_sample.any()
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(),
                      what=f"session of {slots} slots, 1.5B bf16, dialogue {i} (cfg {SCALES[i]}, slot {hs[i].slot}) vs generate() alone")
        print(f"slots {slots} dialogue {i} slot {hs[i].slot}: waveform rel RMS {err:.3e}")
        assert err < 1e-2, f"slots {slots}, dialogue {i}: waveform rel RMS {err:.3e}"


# ---- 3. device noise --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sde", [False, True], ids=["ode", "sde"])
def test_session_device_noise_vs_alone(big, sde):
    """The session's default: noise drawn on the device from (noise_seed, frame).  Three dialogues through two slots - the third takes over a
    used slot - each against generate(device_noise=True, noise_seed=s) alone, to 1e-2; once with the ODE solver and once with the SDE one."""
    cfg, m = big
    tok, prompts, forced, _ = _workload(cfg)
    pick, seeds = [3, 1, 4], [1234567, 2 ** 40 + 5, 99]
    with _Solver(m, sde):
        with m.open_session(tokenizer=tok, slots=2, max_context=256) as sess:
            with pytest.raises(ValueError):
                sess.submit(input_ids=prompts[0][None], cfg_scale=2.0, forced_tokens=forced[0], noise=torch.zeros(8, cfg.latent))
            hs = [sess.submit(input_ids=prompts[i][None], cfg_scale=SCALES[i], forced_tokens=forced[i], noise_seed=s) for i, s in zip(pick, seeds)]
            sess.run()
        assert [h.slot for h in hs] == [0, 1, 1]
        for h, i, s in zip(hs, pick, seeds):
            want = m.generate(input_ids=prompts[i][None], tokenizer=tok, cfg_scale=SCALES[i], forced_tokens=forced[i], device_noise=True, noise_seed=s)
            got = h.result()
            assert got.sequences.tolist() == want.sequences.tolist()
            err = rel_rms(got.speech_outputs[0].float().cpu().numpy(), want.speech_outputs[0].float().cpu().numpy(),
                          what=f"session with device noise ({'SDE' if sde else 'ODE'}), 1.5B bf16, dialogue {i} seed {s} vs generate(device_noise=True) alone")
            print(f"device noise {'sde' if sde else 'ode'} dialogue {i}: {err:.3e}")
            assert err < 1e-2, f"dialogue {i}: waveform rel RMS {err:.3e}"


def test_session_voice_and_voice_prefix_submitted_mid_flight(big):
    """submit() while the session runs, with a voice prompt (encoded in submit, on the lanes' streams) and with a prepared voice_prefix
    (restored into the slot's cache row at admission): each against generate() alone with the same voice inputs, to 1e-2."""
    cfg, m = big
    tok, prompts, forced, noise = _workload(cfg)
    g = torch.Generator().manual_seed(71)
    ids = torch.cat([torch.randint(0, 1000, (39,), generator=g), torch.tensor([tok.speech_start_id])])
    voice = 0.1 * torch.randn(1, 2 * cfg.hop - 321, generator=g)
    sp_mask = torch.zeros(40, dtype=torch.bool)
    sp_mask[7:9] = True
    sm = torch.ones(1, 2, dtype=torch.bool)
    speech_noise = (torch.randn(1, generator=g), torch.randn(1, 2, cfg.ac_dim, generator=g))
    P = 12
    vp = m.prepare_voice_prefix(ids[:P], voice, sm, sp_mask[:P], speech_noise=speech_noise)
    base = dict(input_ids=ids[None], speech_input_mask=sp_mask[None], cfg_scale=2.0, forced_tokens=forced[3], noise=noise[3])
    full = dict(base, speech_tensors=voice, speech_masks=sm, speech_noise=speech_noise)
    with m.open_session(tokenizer=tok, slots=2, max_context=256, device_noise=False) as sess:
        h0 = sess.submit(input_ids=prompts[0][None], cfg_scale=1.3, forced_tokens=forced[0], noise=noise[0])
        assert sess.step() and sess.step()
        hv = sess.submit(**full)
        hp = sess.submit(voice_prefix=vp, **base)
        sess.run()
    assert h0.done and (hv.slot, hp.slot) == (1, 1)
    for name, h, want in (("voice prompt", hv, m.generate(tokenizer=tok, **full)), ("voice_prefix", hp, m.generate(tokenizer=tok, voice_prefix=vp, **base))):
        got = h.result()
        assert got.sequences.tolist() == want.sequences.tolist()
        err = rel_rms(got.speech_outputs[0].float().cpu().numpy(), want.speech_outputs[0].float().cpu().numpy(),
                      what=f"session, 1.5B bf16, a dialogue with a {name} submitted mid-flight vs generate() alone")
        print(f"mid-flight {name}: {err:.3e}")
        assert err < 1e-2, f"{name}: waveform rel RMS {err:.3e}"


# ---- 4. sampling ------------------------------------------------------------------------------------------------------------------
def test_session_device_sampling(big):
    """do_sample with the tokens drawn on the device (one sampler per session), seeded: every token stays inside the constrained vocabulary,
    every dialogue finishes (EOS or its step limit), and two identical session runs give equal sequences."""
    cfg, m = big
    tok, prompts, _, _ = _workload(cfg)
    valid = {tok.speech_start_id, tok.speech_end_id, tok.speech_diffusion_id, tok.eos_token_id}
    runs = []
    for _ in range(2):
        torch.manual_seed(77)
        with m.open_session(tokenizer=tok, slots=3, max_context=256, generation_config={"do_sample": True, "temperature": 1.0, "top_p": 0.95},
                            device_sampling=True) as sess:
            hs = [sess.submit(input_ids=prompts[i][None], cfg_scale=SCALES[i], max_new_tokens=6, noise_seed=500 + i) for i in range(5)]
            n = 0
            while sess.step():
                n += 1
                assert n < 64
        assert all(h.done for h in hs)
        runs.append([h.result().sequences[0].tolist() for h in hs])
    for i, seq in enumerate(runs[0]):
        new = seq[LENS[i]:]
        assert seq[:LENS[i]] == prompts[i].tolist() and 1 <= len(new) <= 6 and set(new) <= valid, (i, new)
        assert len(new) == 6 or new[-1] == tok.eos_token_id
    assert runs[0] == runs[1]


# ---- 5. generate(cfg_scale=[...]) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_batch", [True, False], ids=["rows", "lanes"])
def test_generate_with_a_guidance_scale_per_dialogue(big, row_batch):
    """generate(cfg_scale=[1.3, 3.0, 2.0]) on three dialogues, row-batched (the graph H that reads the scales on the device) and on the lanes
    (each lane its own scalar): every dialogue agrees with the scalar-cfg_scale call on it alone to 1e-2."""
    cfg, m = big
    tok, prompts, forced, noise = _workload(cfg)
    pick, scales = [3, 4, 7], [1.3, 3.0, 2.0]
    Lp = max(LENS[i] for i in pick)
    ids = torch.stack([torch.cat([torch.full((Lp - LENS[i],), tok.pad_id), prompts[i]]) for i in pick])
    mask = torch.stack([torch.cat([torch.zeros(Lp - LENS[i], dtype=torch.long), torch.ones(LENS[i], dtype=torch.long)]) for i in pick])
    out = m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=scales, forced_tokens=[forced[i] for i in pick],
                     noise=torch.stack([noise[i] for i in pick]), row_batch=row_batch)
    if row_batch:
        assert ("Hc",) in m._rowbatch[(3, 0)]._graphs and not any(k[0] == "H" for k in m._rowbatch[(3, 0)]._graphs)
    with pytest.raises(ValueError):
        m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=[1.3, 3.0], forced_tokens=[forced[i] for i in pick])
    for j, i in enumerate(pick):
        want = m.generate(input_ids=prompts[i][None], tokenizer=tok, cfg_scale=scales[j], forced_tokens=forced[i], noise=noise[i])
        assert out.sequences[j, Lp - LENS[i]: Lp + len(forced[i])].tolist() == want.sequences[0].tolist()
        err = rel_rms(out.speech_outputs[j].float().cpu().numpy(), want.speech_outputs[0].float().cpu().numpy(),
                      what=f"generate(cfg_scale=[...]) 1.5B bf16, {'row-batched' if row_batch else 'lanes'}, dialogue {i} at {scales[j]} vs the scalar call alone")
        print(f"cfg list {'rows' if row_batch else 'lanes'} dialogue {i}: {err:.3e}")
        assert err < 1e-2, f"dialogue {i}: waveform rel RMS {err:.3e}"


# ---- 6. the default path ------------------------------------------------------------------------------------------------------------
def test_default_path_untouched_after_a_session(big):
    """After a session has opened and closed on the model, generate() on 4 dialogues with a scalar scale captures the graphs it always did:
    the scale in graph H's key, the old entry point behind it."""
    cfg, m = big
    tok, prompts, forced, noise = _workload(cfg)
    with m.open_session(tokenizer=tok, slots=4, max_context=256) as sess:
        h = sess.submit(input_ids=prompts[6][None], cfg_scale=1.3, forced_tokens=forced[6], noise_seed=3)
        sess.run()
    assert h.done and m._session is None
    pick = [3, 4, 6, 7]
    Lp = max(LENS[i] for i in pick)
    ids = torch.stack([torch.cat([torch.full((Lp - LENS[i],), tok.pad_id), prompts[i]]) for i in pick])
    mask = torch.stack([torch.cat([torch.zeros(Lp - LENS[i], dtype=torch.long), torch.ones(LENS[i], dtype=torch.long)]) for i in pick])
    out = m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=[forced[i] for i in pick],
                     noise=torch.stack([noise[i] for i in pick]))
    rb = m._rowbatch[(4, 0)]
    keys = set(rb._graphs)
    assert ("A", tok.speech_start_id, tok.speech_diffusion_id) in keys and ("H", 2.0) in keys and all(k[0] in ("A", "H") for k in keys), keys
    assert not rb.cfg_rows and all(math.isfinite(float(o.float().abs().max())) for o in out.speech_outputs)
