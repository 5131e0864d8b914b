"""GPU parity of WIDE row batches (row_batch_width=8: 5..8 dialogues, 10..16 rows, in one pass over the LLM and head weights on
gemv_rows16_kernel): the composites at R = 10 / 16 and B = 5 / 8 against their batch-2 and single-utterance forms, generate() and a serving
session on a width-8 model against the lanes and against each dialogue alone.  Every bar is the one the 8-row tests hold the same comparison to
(tests/test_hip_rowbatch.py, test_hip_rowbatch_sde.py, test_hip_session.py); measured errors go into the parity record."""
import ctypes as C

import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset("1.5b")
    sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, row_batch_width=8)
    m.set_ddpm_inference_steps(20)
    return cfg, sd, m


class _Tok:
    def __init__(self, vocab):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = vocab - 4, vocab - 3, vocab - 2, vocab - 1
        self.bos_token_id = None
        self.pad_id = vocab - 5


def _decode_step(m, cfg, B, lens, s_max):
    """One row-batched decode step of B dialogues (2 B rows, one KV cache) against the batch-2 step of every dialogue on the engine's own state:
    hidden rows and constrained logits < 5e-3, same tokens and positions (the comparison of test_decode_step_8_rows_vs_batch2)"""
    from vibevoice_rocm_amd.rowbatch import RowBatch
    tok = _Tok(cfg.vocab)
    ST, SD = tok.speech_start_id, tok.speech_diffusion_id
    valid = [ST, tok.speech_end_id, SD, tok.eos_token_id]
    lanes = [m._lane(b) for b in range(B)]
    rb = RowBatch(lanes)
    g = torch.Generator().manual_seed(17 + B)
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([ST])]) for n in lens]
    rb.begin(s_max, valid, 2.0)
    ref_h, ref_tok, ref_logits, ref_lens = [], [], [], []
    eng = m.engine
    for b in range(B):
        eng.begin_sequence(s_max, valid)
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
                     what=f"row-batched decode step 1.5B, {2 * B} rows, s_max {s_max}, dialogue {b}: hidden rows vs the batch-2 step")
        el = rel_rms(rb.logits[b, :4].cpu().numpy(), ref_logits[b].cpu().numpy())
        assert eh < 5e-3 and el < 5e-3, f"dialogue {b}: hidden {eh:.3e} logits {el:.3e}"
        assert toks[b] == ref_tok[b]
        assert rb.lens[2 * b: 2 * b + 2].tolist() == ref_lens[b].tolist()
    rb.close()


@pytest.mark.parametrize("B", [5, 8])
def test_decode_step_wide_vs_batch2(big, B):
    cfg, sd, m = big
    _decode_step(m, cfg, B, [50, 37, 44, 29, 41, 33, 48, 30][:B], 128)


def test_decode_step_long_context_splits_its_keys(big):
    """R = 10 with s_max = 2048 and ~1100 keys per dialogue.  vv_llm_forward's choice of the split-key attention has no query hook, so the split is
    asserted through what it needs: vv_llm_ws_bytes(m, 10) holds partials and tickets for 16 rows where vv_llm_ws_bytes(m, 8) holds them for 8
    (the workspace the split path writes; before, R > 8 switched the split off) - and the step agrees with the batch-2 steps, which split."""
    cfg, sd, m = big
    lb, llm = m.engine.lib, m.engine.w.llm
    al = lambda n: (4 * n + 255) // 256 * 256
    qkv = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
    rows = lambda R: al(R * cfg.hidden) + al(R * qkv) + al(R * cfg.heads * cfg.head_dim) + al(R * cfg.inter) + al(R * cfg.head_dim)
    att = lambda r: al(r * cfg.heads * 128 * (cfg.head_dim + 2)) + al(r * cfg.heads)
    grow = lb.vv_llm_ws_bytes(C.byref(llm), 10) - lb.vv_llm_ws_bytes(C.byref(llm), 8)
    assert grow == rows(10) - rows(8) + att(16) - att(8), grow
    _decode_step(m, cfg, 5, [1100, 1087, 1093, 1079, 1101], 2048)


def _head_inputs(cfg, B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(2 * B, cfg.hidden, generator=g).cuda(), torch.randn(B, cfg.latent, generator=g).cuda(), g


def _single(eng, cond, noise, b, scale, sde_noise=None):
    cfg = eng.cfg
    one = torch.zeros(cfg.latent, device="cuda")
    with torch.cuda.stream(eng.stream):
        eng._ck(eng.lib.vv_head_sample(C.byref(eng.w.head), cond[2 * b:].data_ptr(), cfg.hidden, noise[b].data_ptr(), eng.temb.data_ptr(), eng._coefs, eng.n_steps,
                                       scale, one.data_ptr(), eng._head_ws.data_ptr(), None if sde_noise is None else sde_noise[b].data_ptr(), eng.sp), "vv_head_sample")
    eng.stream.synchronize()
    return one


@pytest.mark.parametrize("B", [5, 8])
def test_head_sample_batch_wide_vs_single(big, B):
    """vv_head_sample_batch and vv_head_sample_batch_cfg (10 / 16 rows per head matrix pass) against vv_head_sample per utterance: < 2e-3"""
    from test_hip_session import _head_rows, _head_scalar
    cfg, sd, m = big
    eng = m.engine
    eng.w.ensure_frag()
    cond, noise, _ = _head_inputs(cfg, B, 11 + B)
    scales = [1.3, 2.0, 3.0, 2.0, 1.3, 3.0, 1.3, 2.0][:B]
    lat = _head_scalar(eng, cond, noise, None, B, 2.0)
    lat_rows = _head_rows(eng, cond, noise, None, B, scales)
    for b in range(B):
        e = rel_rms(lat[b].cpu().numpy(), _single(eng, cond, noise, b, 2.0).cpu().numpy(),
                    what=f"row-batched head sampling 1.5B, utterance {b} of {B}, vs the single-utterance sampler")
        ec = rel_rms(lat_rows[b].cpu().numpy(), _single(eng, cond, noise, b, scales[b]).cpu().numpy(),
                     what=f"row-batched head sampling 1.5B with guidance rows, utterance {b} of {B}, vs the single-utterance sampler")
        assert e < 2e-3 and ec < 2e-3, f"utterance {b}: rel RMS {e:.3e} (scalar guidance) {ec:.3e} (guidance rows)"


@pytest.mark.parametrize("B", [5, 8])
def test_head_sample_batch_sde_wide_vs_single(big, B):
    from test_hip_rowbatch_sde import _sample_batch_sde, _sde_scheduler
    cfg, sd, m = big
    ode = m.model.noise_scheduler
    m.model.noise_scheduler = _sde_scheduler(ode)
    m.set_ddpm_inference_steps(20)
    try:
        eng = m.engine
        assert eng.sde and eng._coefs[0].cn > 0
        eng.w.ensure_frag()
        cond, noise, g = _head_inputs(cfg, B, 100 + B)
        sde_noise = torch.randn(B, eng.n_steps, cfg.latent, generator=g).cuda()
        lat = _sample_batch_sde(eng, cond, noise, sde_noise, B, 2.0)
        for b in range(B):
            e = rel_rms(lat[b].cpu().numpy(), _single(eng, cond, noise, b, 2.0, sde_noise).cpu().numpy(),
                        what=f"row-batched SDE head sampling 1.5B, utterance {b} of {B}, vs the single-utterance sampler")
            assert e < 2e-3, f"utterance {b}: rel RMS {e:.3e}"
    finally:
        m.model.noise_scheduler = ode
        m.set_ddpm_inference_steps(20)


def test_head_sample_batch_7b_dimensions_fall_back():
    """B = 5 at the 7B head's dimensions (D = 3584: the modulated gate / up GEMV has K > 2048, which the 16-row kernel does not take) - the call
    falls back to the row-major bf16 matrices through vv_linear, as the 8-row path does, at the same bar"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import dataclasses
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    big7 = VVConfig.preset("7b")
    cfg = dataclasses.replace(big7, layers=1)          # the head (and its conditioning width) is the 7B one; one LLM layer keeps the weights small
    sd = synth_state_dict_torch(cfg, 777, device="cuda:0", dtype=torch.bfloat16)
    eng = Engine(cfg, sd, device="cuda:0", dtype=torch.bfloat16)
    eng.set_steps(10)
    eng.w.ensure_frag()
    from test_hip_session import _head_scalar
    B = 5
    cond, noise, _ = _head_inputs(cfg, B, 7)
    lat = _head_scalar(eng, cond, noise, None, B, 2.0)
    for b in range(B):
        e = rel_rms(lat[b].cpu().numpy(), _single(eng, cond, noise, b, 2.0).cpu().numpy(),
                    what=f"row-batched head sampling at 7B head dimensions, utterance {b} of 5, vs the single-utterance sampler")
        assert e < 2e-3, f"utterance {b}: rel RMS {e:.3e}"
    del eng
    torch.cuda.empty_cache()


def test_tail_batch_sample_rows_8_dialogues_vs_single(big):
    """vv_llm_tail_batch_sample_rows at B = 8 against 8 calls of vv_llm_tail_sample_rows: same tokens, positions and frame counters"""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.engine import write_sampler_row
    cfg, sd, m = big
    eng = m.engine
    lb, B, H, nv = eng.lib, 8, cfg.hidden, 4
    tok = _Tok(cfg.vocab)
    ids = [tok.speech_start_id, tok.speech_end_id, tok.speech_diffusion_id, tok.eos_token_id]
    g = torch.Generator().manual_seed(5)
    h = torch.randn(2 * B, H, generator=g).cuda()
    idd = torch.tensor(ids, dtype=torch.int32, device="cuda")
    wv = torch.empty(nv, H, dtype=torch.bfloat16, device="cuda")
    L.check(lb.vv_gather_rows(eng.w.lm_head.data_ptr(), eng.w.wdt, H, (C.c_int * nv)(*ids), nv, wv.data_ptr(), None), "vv_gather_rows")
    smp = torch.zeros(B, 3, dtype=torch.float32)
    for b in range(B):
        write_sampler_row(smp, b, 0.7 + 0.1 * b, 0 if b % 2 else 3, 0.9)
    smp = smp.cuda()
    seeds = torch.arange(1000, 1000 + B, dtype=torch.int64, device="cuda")
    none = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    res = {}
    for form in ("batch", "single"):
        out = torch.zeros(2 * B, H, device="cuda")
        logits = torch.zeros(B, 8, device="cuda")
        toks = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        lens = torch.arange(40, 40 + 2 * B, dtype=torch.int32, device="cuda")
        frame = torch.zeros(B, dtype=torch.int32, device="cuda")
        if form == "batch":
            L.check(lb.vv_llm_tail_batch_sample_rows(C.byref(eng.w.llm), h.data_ptr(), H, B, out.data_ptr(), H, wv.data_ptr(), nv, idd.data_ptr(), logits.data_ptr(),
                                                     toks.data_ptr(), none.data_ptr(), lens.data_ptr(), ids[0], ids[2], frame.data_ptr(), None, smp.data_ptr(),
                                                     seeds.data_ptr(), None), "vv_llm_tail_batch_sample_rows")
        else:
            for b in range(B):
                L.check(lb.vv_llm_tail_sample_rows(C.byref(eng.w.llm), h[2 * b:].data_ptr(), H, 2, out[2 * b:].data_ptr(), H, wv.data_ptr(), nv, idd.data_ptr(),
                                                   logits[b].data_ptr(), toks[b:].data_ptr(), none.data_ptr(), lens[2 * b:].data_ptr(), ids[0], ids[2],
                                                   frame[b:].data_ptr(), smp[b].data_ptr(), seeds[b:].data_ptr(), None), "vv_llm_tail_sample_rows")
        torch.cuda.synchronize()
        res[form] = (toks.tolist(), lens.tolist(), frame.tolist(), logits[:, :nv].cpu())
    assert res["batch"][:3] == res["single"][:3], (res["batch"][:3], res["single"][:3])
    assert all(t in ids for t in res["batch"][0])
    assert torch.equal(res["batch"][3], res["single"][3])


def _dialogues(cfg, B, seed):
    tok = _Tok(cfg.vocab)
    D, E, EOS, S = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id, tok.speech_start_id
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.cat([torch.randint(0, 1000, (39,), generator=g), torch.tensor([S])]) for _ in range(B)])
    # different schedules: 0 ends early, 1 switches turns (a speculated frame is rolled back), the rest run 3..5 frames
    forced = [[D] * (2 if b == 0 else 3 + (b % 3)) + ([E, S, D, D] if b == 1 else []) + [E, EOS] for b in range(B)]
    noise = torch.randn(B, 8, cfg.latent, generator=g)
    return tok, dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)


@pytest.mark.parametrize("B", [6, 10])
def test_generate_wide_row_batches_vs_lanes(big, B):
    """generate(row_batch_width=8) on 6 dialogues (one wide batch) and on 10 (5 + 5) against the lanes: same sequences, waveforms < 1e-2; then
    a default-width call in the same process still builds today's partition"""
    cfg, sd, m = big
    tok, kw = _dialogues(cfg, B, 37 + B)
    before = set(m._rowbatch)
    rows = m.generate(row_batch=True, row_batch_width=8, **kw)
    lanes = m.generate(row_batch=False, **kw)
    want = [(6, 0, "side")] if B == 6 else [(5, 0, "side"), (5, 5, "side")]
    assert all(k in m._rowbatch for k in want) and set(m._rowbatch) - before <= set(want), sorted(map(str, m._rowbatch))
    assert rows.sequences.tolist() == lanes.sequences.tolist()
    for b in range(B):
        assert rows.speech_outputs[b].shape == lanes.speech_outputs[b].shape
        err = rel_rms(rows.speech_outputs[b].float().cpu().numpy(), lanes.speech_outputs[b].float().cpu().numpy(),
                      what=f"generate() on {B} dialogues (row_batch_width=8) 1.5B bf16 vs lanes, waveform of dialogue {b}")
        assert err < 1e-2, f"{B} dialogues, dialogue {b}: waveform rel RMS {err:.3e}"
    if B == 6:
        narrow = m.generate(row_batch=True, row_batch_width=4, **kw)
        assert (3, 0, "side") in m._rowbatch and (3, 3, "side") in m._rowbatch
        assert narrow.sequences.tolist() == lanes.sequences.tolist()


def test_generate_wide_device_noise_and_seeded_tokens(big):
    """One wide-batch call (6 dialogues) with device_noise=True, seeded_tokens=True: dialogue 2 samples its tokens and draws the same tokens and
    the same waveform (< 1e-2) as alone.  Its neighbours follow forced schedules without a frame, as in tests/test_hip_token_seed.py: a batched call
    couples its dialogues where the reference's loop does (a neighbour's first frame restarts the others' conv state), which no seed undoes."""
    cfg, sd, m = big
    tok = _Tok(cfg.vocab)
    ST, SE, EOS = tok.speech_start_id, tok.speech_end_id, tok.eos_token_id
    g = torch.Generator().manual_seed(91)
    B, me = 6, 2
    ids = torch.stack([torch.cat([torch.randint(0, 1000, (31,), generator=g), torch.tensor([ST])]) for _ in range(B)])
    gen = {"do_sample": True, "temperature": 1.0, "top_p": 0.95}
    forced = [None if b == me else ([ST, SE] if b % 2 else [SE, ST]) * (3 + b) + [EOS] for b in range(B)]
    kw = dict(tokenizer=tok, cfg_scale=1.5, max_new_tokens=9, device_noise=True, seeded_tokens=True)
    wide = m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), noise_seed=[700 + b for b in range(B)], token_seed=[900 + b for b in range(B)],
                      generation_config=[gen if b == me else {"do_sample": False} for b in range(B)], forced_tokens=forced, row_batch=True,
                      row_batch_width=8, **kw)
    assert (6, 0, "side") in m._rowbatch
    alone = m.generate(input_ids=ids[me][None], noise_seed=700 + me, token_seed=900 + me, generation_config=gen, **kw)
    want = alone.sequences[0, ids.shape[1]:].tolist()
    got = wide.sequences[me, ids.shape[1]:].tolist()
    print("sampled tokens alone", want, "in the wide batch", got)
    assert got[: len(want)] == want
    a, r = wide.speech_outputs[me], alone.speech_outputs[0]
    assert (a is None) == (r is None)
    if a is not None:
        assert a.shape == r.shape
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what="wide row batch with device noise and seeded tokens, the sampled dialogue vs alone")
        assert err < 1e-2, f"waveform rel RMS {err:.3e}"


def test_session_of_8_slots_is_one_wide_row_batch(big):
    """open_session(slots=8) on a width-8 model: one row batch of 8.  Ten requests of different lengths, so that slots are refilled; each against
    generate() on it alone: same sequence, waveform < 1e-2"""
    cfg, sd, m = big
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(61)
    lens = [50, 37, 44, 29, 41, 33, 48, 30, 36, 45]
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([S])]) for n in lens]
    forced = [[D] * (2 + (3 * i) % 5) + ([E, S, D, D] if i == 2 else []) + [E, EOS] for i in range(10)]
    noise = torch.randn(10, 8, cfg.latent, generator=g)
    scales = [1.3, 2.0, 3.0, 2.0, 1.3, 3.0, 1.3, 2.0, 3.0, 2.0]
    with m.open_session(tokenizer=tok, slots=8, max_context=256, device_noise=False) as sess:
        assert [len(idxs) for _, idxs in sess.driver.groups] == [8] and (8, 0, "session", "side") in m._rowbatch
        hs = [sess.submit(input_ids=prompts[i][None], cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i]) for i in range(10)]
        sess.run()
        got = [h.result() for h in hs]
        assert len({h.slot for h in hs}) < 10          # a slot served more than one request
    for i in range(10):
        want = m.generate(input_ids=prompts[i][None], tokenizer=tok, cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i])
        assert got[i].sequences.tolist() == want.sequences.tolist(), i
        err = rel_rms(got[i].speech_outputs[0].float().cpu().numpy(), want.speech_outputs[0].float().cpu().numpy(),
                      what=f"session of 8 slots (one wide row batch), request {i} vs generate() alone")
        assert err < 1e-2, f"request {i}: waveform rel RMS {err:.3e}"
