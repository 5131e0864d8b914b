"""Device-side do_sample (vv_sampler in include/vv_hip.h): the sampling forms of the LLM step tail and of the first-token pick against the host
sampler's arithmetic on the kernels' own fp32 logits and the same exponential draws, and generate(do_sample=True, device_sampling=True) against
the host-sampler path of the same seeded call - tokens, generator state, chunk delivery, waveforms, and which host round trips are gone."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

TEMPS, TOP_PS, TOP_KS, SCALES = (0.6, 0.95, 1.0, 1.3), (0.5, 0.85, 0.95, 1.0), (0, 2, 3), (0.5, 2.0, 6.0)
SKIP_CAP = 0.01          # at most 1 % of a parametrisation's cases may sit within rounding of a tie on the host


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    lb = L.load()
    L.check(lb.vv_init(), "vv_init")
    return lb


def _llm(hidden, wdt, norm_w, eps=1e-6):
    from vibevoice_rocm_amd import _lib as L
    m = L.Llm()
    m.wdt, m.hidden, m.rms_eps, m.final_norm = wdt, hidden, eps, norm_w.data_ptr()
    return m


def _draw_samplers(n, rng):
    """n samplers from the grid; the values are the fp32 ones the vv_sampler struct holds, so host and device see the same numbers"""
    return [(float(np.float32(rng.choice(TEMPS))), int(rng.choice(TOP_KS)), float(np.float32(rng.choice(TOP_PS)))) for _ in range(n)]


def _host_choice(logits, q, smp):
    """(index the host sampler's arithmetic picks for these fp32 logits and draws, near_tie): modeling._warped_probs, then argmax(p / q) in
    fp32.  near_tie: the host computation itself is within rounding of a tie - best / second-best of p / q closer than 1e-5 relative, a
    cumulative probability within 1e-8 of 1 - top_p, or the k-th and (k + 1)-th logit closer than 1e-5."""
    from vibevoice_rocm_amd.modeling import _warped_probs
    temperature, top_k, top_p = smp
    v = _warped_probs(dict(temperature=temperature, top_k=top_k, top_p=top_p))(logits.clone()) / q
    srt = torch.sort(v, descending=True).values
    tie = bool(srt[0] - srt[1] < 1e-5 * srt[0])
    z = logits.double() / temperature
    if 0 < top_k < z.numel():
        ls = torch.sort(logits, descending=True).values
        tie = tie or bool(ls[top_k - 1] - ls[top_k] < 1e-5)
        z = torch.where(z < torch.topk(z, top_k).values[-1], torch.full_like(z, float("-inf")), z)
    if top_p < 1.0:
        cum = torch.softmax(torch.sort(z).values, -1).cumsum(-1)
        tie = tie or bool(((cum - (1 - top_p)).abs() < 1e-8).any())
    return int(torch.argmax(v)), tie


def _tail_is_fast(R, nv, hidden, ldh, ldo, h_ptr, out_ptr, w_ptr, bf16):
    """the dispatch condition of vv_llm_tail(_sample) restated: True = llm_tail_fast_kernel, False = the general LDS kernel"""
    return (R <= 2 and nv <= 8 and hidden % 4 == 0 and hidden <= 4096 and h_ptr % 16 == 0 and ldh % 4 == 0 and out_ptr % 16 == 0
            and ldo % 4 == 0 and w_ptr % (8 if bf16 else 16) == 0)


N_DRAWS = 300


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("nv", [4, 5])
@pytest.mark.parametrize("hidden,ldh_pad,fast", [(64, 1, False), (64, 0, True), (1536, 0, True), (1536, 1, False)])
def test_llm_tail_sample_vs_host_sampler(lib, hidden, ldh_pad, fast, nv, bf16):
    """vv_llm_tail_sample, R = 2, on the fast kernel (aligned rows) and the general one (odd row stride): 300 (h, q, sampler) draws with logit
    scales 0.5 / 2 / 6.  The token equals what the host sampler's arithmetic picks from the kernel's own logits_out and the same q; out,
    logits_out, lens and frame_counter are bit-identical to vv_llm_tail with that token forced."""
    from vibevoice_rocm_amd import _lib as L
    gen = torch.Generator().manual_seed(hidden + 7 * nv + bf16 + ldh_pad)
    rng = np.random.default_rng(hidden + nv + 2 * bf16 + ldh_pad)
    norm_w = (1 + 0.1 * torch.randn(hidden, generator=gen)).cuda()
    m = _llm(hidden, L.VV_BF16 if bf16 else L.VV_F32, norm_w)
    ldh = hidden + ldh_pad
    w = torch.randn(nv, hidden, generator=gen) / np.sqrt(hidden)
    ws = [((w * s).to(torch.bfloat16) if bf16 else w * s).cuda() for s in SCALES]
    ids = rng.permutation(np.arange(300, 300 + nv)).astype(np.int32)
    idd = torch.from_numpy(ids).cuda()
    N = N_DRAWS
    samplers = _draw_samplers(N, rng)
    H = (torch.randn(N, 2, ldh, generator=gen) * 2).cuda()
    Q = torch.empty(N, nv).exponential_(1, generator=gen)
    Qd = Q.cuda()
    lens0 = torch.from_numpy(rng.integers(1, 40, (N, 2)).astype(np.int32)).cuda()
    frame0 = torch.from_numpy(rng.integers(0, 5, N).astype(np.int32)).cuda()
    none = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    res = {}
    for form in ("sample", "argmax"):
        out = torch.full((N, 2, hidden), float("nan"), device="cuda")
        logits = torch.full((N, 8), float("nan"), device="cuda")
        tok = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        lens, frame = lens0.clone(), frame0.clone()
        for n in range(N):
            wd = ws[n % 3]
            assert _tail_is_fast(2, nv, hidden, ldh, hidden, H[n].data_ptr(), out[n].data_ptr(), wd.data_ptr(), bf16) == fast
            # tok_start / tok_diffusion are ids of the set in turn: every bookkeeping branch is taken by some draw
            ts, td = int(ids[n % nv]), int(ids[(n + 1) % nv])
            a = (C.byref(m), H[n].data_ptr(), ldh, 2, out[n].data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(), logits[n].data_ptr(),
                 tok[n:].data_ptr())
            if form == "sample":
                smp = L.Sampler(*samplers[n])
                L.check(lib.vv_llm_tail_sample(*a, none.data_ptr(), lens[n].data_ptr(), ts, td, frame[n:].data_ptr(), C.byref(smp), Qd[n].data_ptr(), None),
                        "vv_llm_tail_sample")
            else:
                L.check(lib.vv_llm_tail(*a, res["sample"][2][n:].data_ptr(), lens[n].data_ptr(), ts, td, frame[n:].data_ptr(), None), "vv_llm_tail")
        torch.cuda.synchronize()
        res[form] = (out, logits, tok, lens, frame)
    for a, b, what in zip(res["sample"], res["argmax"], ("out", "logits_out", "token", "lens", "frame_counter")):
        assert torch.equal(a[:, :nv] if what == "logits_out" else a, b[:, :nv] if what == "logits_out" else b), what
    assert not bool((res["sample"][3] == lens0).all())
    lg, tk = res["sample"][1].cpu()[:, :nv], res["sample"][2].cpu()
    skipped = 0
    for n in range(N):
        i, tie = _host_choice(lg[n], Q[n], samplers[n])
        if tie:
            skipped += 1
            continue
        assert int(tk[n]) == int(ids[i]), (n, samplers[n], lg[n], Q[n], int(tk[n]), int(ids[i]))
    assert skipped <= SKIP_CAP * N, skipped
    assert len(set(tk.tolist())) == nv          # every id is drawn by some case


def test_llm_tail_batch_sample_vs_host_sampler(lib):
    """vv_llm_tail_batch_sample, B = 3 (hidden 1536, bf16, nv 5): dialogue 0 draws, dialogue 1 is inactive (draws a token, positions stay),
    dialogue 2 is forced (its q row is garbage: NaN).  Tokens against the host arithmetic on the kernel's logits; everything bit-identical to
    vv_llm_tail_batch with the tokens forced."""
    from vibevoice_rocm_amd import _lib as L
    hidden, nv, B, N = 1536, 5, 3, N_DRAWS
    gen = torch.Generator().manual_seed(91)
    rng = np.random.default_rng(91)
    norm_w = (1 + 0.1 * torch.randn(hidden, generator=gen)).cuda()
    m = _llm(hidden, L.VV_BF16, norm_w)
    w = torch.randn(nv, hidden, generator=gen) / np.sqrt(hidden)
    ws = [(w * s).to(torch.bfloat16).cuda() for s in SCALES]
    ids = rng.permutation(np.arange(500, 500 + nv)).astype(np.int32)
    idd = torch.from_numpy(ids).cuda()
    samplers = _draw_samplers(N, rng)
    H = (torch.randn(N, 2 * B, hidden, generator=gen) * 2).cuda()
    Q = torch.ones(N, B, 8)
    Q[:, :, :nv] = torch.empty(N, B, nv).exponential_(1, generator=gen)
    Q[:, 2] = float("nan")
    Qd = Q.cuda()
    forced = torch.full((N, B), -1, dtype=torch.int32)
    forced[:, 2] = torch.from_numpy(rng.choice(ids, N).astype(np.int32))
    fd = forced.cuda()
    active = torch.tensor([1, 0, 1], dtype=torch.int32, device="cuda")
    lens0 = torch.from_numpy(rng.integers(1, 40, (N, 2 * B)).astype(np.int32)).cuda()
    frame0 = torch.from_numpy(rng.integers(0, 5, (N, B)).astype(np.int32)).cuda()
    res = {}
    for form in ("sample", "argmax"):
        out = torch.full((N, 2 * B, hidden), float("nan"), device="cuda")
        logits = torch.full((N, B, 8), float("nan"), device="cuda")
        tok = torch.full((N, B), -7, dtype=torch.int32, device="cuda")
        lens, frame = lens0.clone(), frame0.clone()
        for n in range(N):
            ts, td = int(ids[n % nv]), int(ids[(n + 1) % nv])
            a = (C.byref(m), H[n].data_ptr(), hidden, B, out[n].data_ptr(), hidden, ws[n % 3].data_ptr(), nv, idd.data_ptr(), logits[n].data_ptr(),
                 tok[n].data_ptr())
            b = (lens[n].data_ptr(), ts, td, frame[n].data_ptr(), active.data_ptr())
            if form == "sample":
                smp = L.Sampler(*samplers[n])
                L.check(lib.vv_llm_tail_batch_sample(*a, fd[n].data_ptr(), *b, C.byref(smp), Qd[n].data_ptr(), None), "vv_llm_tail_batch_sample")
            else:
                L.check(lib.vv_llm_tail_batch(*a, res["sample"][2][n].data_ptr(), *b, None), "vv_llm_tail_batch")
        torch.cuda.synchronize()
        res[form] = (out, logits, tok, lens, frame)
    for a, b, what in zip(res["sample"], res["argmax"], ("out", "logits_out", "token", "lens", "frame_counter")):
        assert torch.equal(a[..., :nv] if what == "logits_out" else a, b[..., :nv] if what == "logits_out" else b), what
    lg, tk = res["sample"][1].cpu(), res["sample"][2].cpu()
    assert torch.equal(tk[:, 2], forced[:, 2])                                    # the forced dialogue ignores its (NaN) q row
    assert torch.equal(res["sample"][3][:, 2:4], lens0[:, 2:4]) and torch.equal(res["sample"][4][:, 1], frame0[:, 1])     # inactive: positions stay
    assert bool((res["sample"][3][:, 0] == lens0[:, 0] + 1).all()) and bool((res["sample"][3][:, 4] == lens0[:, 4] + 1).all())
    skipped = 0
    for n in range(N):
        for b in (0, 1):
            i, tie = _host_choice(lg[n, b, :nv], Q[n, b, :nv], samplers[n])
            if tie:
                skipped += 1
                continue
            assert int(tk[n, b]) == int(ids[i]), (n, b, samplers[n])
    assert skipped <= SKIP_CAP * 2 * N, skipped


@pytest.mark.parametrize("nv", [4, 5])
def test_sample_ids_vs_host_sampler(lib, nv):
    """vv_sample_ids (the first token after the prefill) on 300 (logits, q, sampler) draws; a forced token wins over a NaN q."""
    from vibevoice_rocm_amd import _lib as L
    gen = torch.Generator().manual_seed(17 + nv)
    rng = np.random.default_rng(17 + nv)
    N = N_DRAWS
    ids = rng.permutation(np.arange(40, 40 + nv)).astype(np.int32)
    idd = torch.from_numpy(ids).cuda()
    samplers = _draw_samplers(N, rng)
    lg = torch.randn(N, nv, generator=gen) * torch.tensor(SCALES).repeat(N // 3 + 1)[:N, None]
    Q = torch.empty(N, nv).exponential_(1, generator=gen)
    lgd, Qd = lg.cuda(), Q.cuda()
    tok = torch.full((N,), -7, dtype=torch.int32, device="cuda")
    for n in range(N):
        smp = L.Sampler(*samplers[n])
        L.check(lib.vv_sample_ids(lgd[n].data_ptr(), nv, idd.data_ptr(), C.byref(smp), Qd[n].data_ptr(), tok[n:].data_ptr(), None, None), "vv_sample_ids")
    torch.cuda.synchronize()
    tk = tok.cpu()
    skipped = 0
    for n in range(N):
        i, tie = _host_choice(lg[n], Q[n], samplers[n])
        if tie:
            skipped += 1
            continue
        assert int(tk[n]) == int(ids[i]), (n, samplers[n], lg[n], Q[n])
    assert skipped <= SKIP_CAP * N, skipped
    f = torch.tensor([int(ids[1])], dtype=torch.int32, device="cuda")
    nan_q = torch.full((8,), float("nan"), device="cuda")
    smp = L.Sampler(0.95, 0, 0.95)
    L.check(lib.vv_sample_ids(lgd[0].data_ptr(), nv, idd.data_ptr(), C.byref(smp), nan_q.data_ptr(), tok.data_ptr(), f.data_ptr(), None), "vv_sample_ids")
    assert int(tok[0].item()) == int(ids[1])


def test_sampling_entries_reject_bad_arguments(lib):
    """temperature <= 0, top_p outside (0, 1], nv > 8, NULL q, NULL sampler: VV_E_ARG from all three entries, nothing launched"""
    from vibevoice_rocm_amd import _lib as L
    hidden = 64
    norm_w = torch.ones(hidden, device="cuda")
    m = _llm(hidden, L.VV_F32, norm_w)
    h, out, w = torch.zeros(6, hidden, device="cuda"), torch.zeros(6, hidden, device="cuda"), torch.zeros(9, hidden, device="cuda")
    ids = torch.arange(9, dtype=torch.int32, device="cuda")
    lg, q, tok = torch.zeros(32, device="cuda"), torch.ones(32, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    good = (1.0, 0, 1.0)
    cases = [((0.0, 0, 1.0), 4, True), ((-1.0, 0, 1.0), 4, True), ((1.0, 0, 0.0), 4, True), ((1.0, 0, 1.5), 4, True), (good, 9, True), (good, 4, False),
             (None, 4, True)]
    for smp, nv, with_q in cases:
        s = None if smp is None else C.byref(L.Sampler(*smp))
        qp = q.data_ptr() if with_q else None
        rcs = [lib.vv_llm_tail_sample(C.byref(m), h.data_ptr(), hidden, 2, out.data_ptr(), hidden, w.data_ptr(), nv, ids.data_ptr(), lg.data_ptr(),
                                      tok.data_ptr(), None, None, 0, 0, None, s, qp, None),
               lib.vv_llm_tail_batch_sample(C.byref(m), h.data_ptr(), hidden, 3, out.data_ptr(), hidden, w.data_ptr(), nv, ids.data_ptr(), lg.data_ptr(),
                                            tok.data_ptr(), None, None, 0, 0, None, None, s, qp, None),
               lib.vv_sample_ids(lg.data_ptr(), nv, ids.data_ptr(), s, qp, tok.data_ptr(), None, None)]
        assert rcs == [-1, -1, -1], (smp, nv, with_q, rcs)          # VV_E_ARG
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
class _Tok:
    def __init__(self, vocab):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = vocab - 4, vocab - 3, vocab - 2, vocab - 1
        self.bos_token_id = None
        self.pad_id = 0


def _drop(m):
    torch.cuda.synchronize()
    m.release_lanes()
    del m
    gc.collect()
    torch.cuda.synchronize()


def _prompts(cfg, lens, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.cat([torch.randint(0, cfg.vocab - 8, (n - 1,), generator=g), torch.tensor([cfg.vocab - 4])]) for n in lens]


def _spy_streamer(B):
    from vibevoice_rocm_amd.streamer import AudioStreamer
    st, ev = AudioStreamer(batch_size=B, timeout=5), []
    put0 = st.put

    def put(chunks, idx):
        ev.append([int(i) for i in idx])
        put0(chunks, idx)
    st.put = put
    return st, ev


def _count(monkeypatch, cls, name, counts):
    real = getattr(cls, name)

    def spy(self, *a, **k):
        counts[name] = counts.get(name, 0) + 1
        return real(self, *a, **k)
    monkeypatch.setattr(cls, name, spy)


SINGLE = dict(seed=0, temperature=1.0, prompt_seed=5, max_new_tokens=24)
BATCH = dict(seed=0, temperature=1.0, prompt_seed=6, max_new_tokens=16)


def test_generate_single_dialogue_device_sampling_vs_host_sampler(monkeypatch):
    """`tiny` fp32 from_synthetic, seeded default generator, no forced tokens, drawn noise, an AudioStreamer: device_sampling=True against the
    host sampler - same tokens, same torch.get_rng_state() afterwards (the noise of the mis-speculated frame is taken back), same chunks in
    number and order, no Engine._host_logits call at all (the host path makes one per sampled token), and frames are speculated: the run
    leaves speech_diffusion (see MISSPEC below), which the rollback spy sees.  Seed 0 (chosen by inspection of the first run) samples
    SD ST SD ST ST SD SE ST ST SD ST EOS: the frames speculated at steps 1, 3, 6 and 10 are rolled back.  Waveforms: the single-launch tail and
    the A1 / A2 pair normalise the hidden row in different kernels, so no bit equality is assumed; bar 1e-2, the lanes-vs-row-batch bar of
    tests/test_hip_rowbatch.py; measured on MI355X: rel RMS 0 (the two paths came out bit-identical here; profiles/device_sampling.txt).
    With do_sample=False the keyword is inert: bit-identical output."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg = VVConfig.preset("tiny")
    tok = _Tok(cfg.vocab)
    SD = tok.speech_diffusion_id
    ids = _prompts(cfg, [24], SINGLE["prompt_seed"])[0]
    gen_cfg = {"do_sample": True, "temperature": SINGLE["temperature"], "top_p": 0.95}
    counts = {}
    _count(monkeypatch, Engine, "_host_logits", counts)
    _count(monkeypatch, Engine, "rollback_speech_state", counts)
    m = VibeVoiceForConditionalGenerationInference.from_synthetic(cfg, seed=1234, device="cuda:0", torch_dtype=torch.float32)
    try:
        m.set_ddpm_inference_steps(5)
        res = {}
        for dev in (False, True):
            counts.clear()
            st, ev = _spy_streamer(1)
            torch.manual_seed(SINGLE["seed"])
            out = m.generate(input_ids=ids[None], tokenizer=tok, cfg_scale=1.3, generation_config=gen_cfg, max_new_tokens=SINGLE["max_new_tokens"],
                             audio_streamer=st, device_sampling=dev)
            res[dev] = (out, torch.get_rng_state(), ev, dict(counts))
        greedy = [m.generate(input_ids=ids[None], tokenizer=tok, cfg_scale=1.3, generation_config={"do_sample": False}, max_new_tokens=8,
                             noise=torch.zeros(8, cfg.latent), device_sampling=dev) for dev in (False, True)]
    finally:
        _drop(m)
    (oh, sh, eh, ch), (od, sd_, ed, cd) = res[False], res[True]
    seq = od.sequences[0, 24:].tolist()
    print("single dialogue, sampled tokens:", seq, "host counts", ch, "device counts", cd)
    assert od.sequences.tolist() == oh.sequences.tolist()
    assert torch.equal(sd_, sh)
    assert ed == eh and len(ed) == seq.count(SD) > 0
    assert cd.get("_host_logits", 0) == 0 and ch["_host_logits"] >= len(seq) - 1
    # MISSPEC: a step whose predecessor is speech_diffusion and whose own token is not - its frame was launched speculatively and rolled back
    misspec = [t for t in range(1, len(seq)) if seq[t - 1] == SD and seq[t] != SD]
    assert misspec and cd.get("rollback_speech_state", 0) == len(misspec) and ch.get("rollback_speech_state", 0) == 0, (seq, cd, ch)
    err = rel_rms(od.speech_outputs[0].float().cpu().numpy(), oh.speech_outputs[0].float().cpu().numpy(),
                  what="generate() tiny fp32 do_sample, device sampler vs host sampler")
    print(f"single dialogue waveform rel RMS device vs host sampler: {err:.3e}")
    assert err < 1e-2, err
    assert greedy[0].sequences.tolist() == greedy[1].sequences.tolist()
    a, b = greedy[0].speech_outputs[0], greedy[1].speech_outputs[0]
    assert (a is None) == (b is None) and (a is None or torch.equal(a, b))


@pytest.mark.parametrize("row_batch", [False, True])
def test_generate_three_dialogues_device_sampling_vs_host_sampler(monkeypatch, row_batch):
    """3 dialogues with different prompts and injected noise, on the lanes and row-batched (`mid` bf16: the row-batched GEMVs do not take
    tiny's hidden 64): tokens, generator state, chunk delivery and waveforms (bar 1e-2) as for the single dialogue; with device_sampling
    neither RowBatch.decode_logits nor Engine._host_logits is called, with the host sampler the path's own one is, once per step.  Seed 0
    (by inspection of the first run): SD SE SD SE EOS / SD SE ST SE SE EOS / EOS - the dialogues end at steps 4, 5 and 0, dialogue 0's frames
    speculated at steps 1 and 3 are rolled back.  Measured on MI355X: waveform rel RMS 0 on both paths (profiles/device_sampling.txt)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.rowbatch import RowBatch
    cfg = VVConfig.preset("mid")
    tok = _Tok(cfg.vocab)
    SD, EOS = tok.speech_diffusion_id, tok.eos_token_id
    lens = [30, 21, 26]
    prompts = _prompts(cfg, lens, BATCH["prompt_seed"])
    Lp = max(lens)
    ids = torch.stack([torch.cat([torch.full((Lp - n,), tok.pad_id), p]) for n, p in zip(lens, prompts)])
    mask = torch.stack([torch.cat([torch.zeros(Lp - n, dtype=torch.long), torch.ones(n, dtype=torch.long)]) for n in lens])
    noise = torch.randn(3, BATCH["max_new_tokens"], cfg.latent, generator=torch.Generator().manual_seed(2))
    gen_cfg = {"do_sample": True, "temperature": BATCH["temperature"], "top_p": 0.95}
    counts = {}
    _count(monkeypatch, Engine, "_host_logits", counts)
    _count(monkeypatch, RowBatch, "decode_logits", counts)
    m = VibeVoiceForConditionalGenerationInference.from_synthetic(cfg, seed=1234, device="cuda:0", torch_dtype=torch.bfloat16)
    try:
        m.set_ddpm_inference_steps(5)
        res = {}
        for dev in (False, True):
            counts.clear()
            st, ev = _spy_streamer(3)
            torch.manual_seed(BATCH["seed"])
            out = m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=1.3, generation_config=gen_cfg, noise=noise,
                             max_new_tokens=BATCH["max_new_tokens"], audio_streamer=st, row_batch=row_batch, device_sampling=dev)
            res[dev] = (out, torch.get_rng_state(), ev, dict(counts))
        assert ((3, 0) in m._rowbatch) == row_batch
    finally:
        _drop(m)
    (oh, sh, eh, ch), (od, sd_, ed, cd) = res[False], res[True]
    seqs = [od.sequences[b, Lp:].tolist() for b in range(3)]
    print("three dialogues, row_batch", row_batch, "tokens:", seqs, "host counts", ch, "device counts", cd)
    assert od.sequences.tolist() == oh.sequences.tolist()
    assert torch.equal(sd_, sh)
    assert ed == eh and ed
    assert cd.get("_host_logits", 0) == 0 and cd.get("decode_logits", 0) == 0
    assert ch.get("decode_logits" if row_batch else "_host_logits", 0) > 0
    ends = [s.index(EOS) if EOS in s else len(s) for s in seqs]
    assert len(set(ends)) > 1, ends                   # the dialogues finish at different steps
    for b in range(3):
        a, r = od.speech_outputs[b], oh.speech_outputs[b]
        assert (a is None) == (r is None)
        if a is not None:
            err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(),
                          what=f"generate() 3 dialogues mid bf16 do_sample, device vs host sampler, row_batch={row_batch}, dialogue {b}")
            print(f"dialogue {b} waveform rel RMS device vs host sampler: {err:.3e}")
            assert err < 1e-2, (b, err)
    assert any(SD in s for s in seqs)
