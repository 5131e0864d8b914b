"""Diffusion noise drawn on the device (vv_noise_normal in include/vv_hip.h; generate(device_noise=True, noise_seed=...)) on the GPU: the kernel
against the float64 evaluation of its definition (tests/philox_ref.py), its argument checks, and generate() with the option - one dialogue,
lanes and row batches - against the same calls with the kernel's own rows injected, bit for bit where the launch sequences are the same."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import philox_ref as P
from conftest import rel_rms

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
SEEDS = (0, 2 ** 64 - 1, 0x0123456789abcdef)
FRAMES = (0, 1, 2 ** 31 - 1)
BAR = 2e-5          # max abs error against the float64 reference: derived bound ~5e-6 (exact uniforms, 2 pi u off by <= 7.5e-7 rad, r <= 6.76,
                    # logf / sinf / cosf to a couple of ulp), a wrong counter or constant is O(1)


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    lb = L.load()
    L.check(lb.vv_init(), "vv_init")
    return lb


def _i64(seeds):
    """64-bit seeds as the int64 tensor that holds their bits"""
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in (int(v) % 2 ** 64 for v in seeds)], dtype=torch.int64)


def _call(lib, B, n, n_steps, seeds, frames, pad=3):
    """one vv_noise_normal call into sentinel-filled buffers with ld_noise = n + pad, ld_sde = n_steps * n + pad: (rc, noise [B, ld], sde [B, ld_sde] or None)"""
    noise = torch.full((B, n + pad), SENTINEL, device="cuda")
    sde = torch.full((B, n_steps * n + pad), SENTINEL, device="cuda") if n_steps else None
    sd, fr = _i64(seeds).cuda(), torch.tensor(frames, dtype=torch.int32).cuda()
    rc = lib.vv_noise_normal(noise.data_ptr(), n + pad, None if sde is None else sde.data_ptr(), n_steps * n + pad, B, n, n_steps, sd.data_ptr(), fr.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, noise.cpu().numpy(), None if sde is None else sde.cpu().numpy()


def _rows(noise, sde, b, n, n_steps):
    """{kind: fp32 [n]} of dialogue b, after checking that its padding columns still hold the sentinel"""
    assert (noise[b, n:] == SENTINEL).all()
    out = {0: noise[b, :n]}
    if sde is not None:
        assert (sde[b, n_steps * n:] == SENTINEL).all()
        for s in range(n_steps):
            out[1 + s] = sde[b, s * n: (s + 1) * n]
    return out


@pytest.mark.parametrize("n_steps", [0, 3])
@pytest.mark.parametrize("n", [64, 6, 1])
def test_noise_kernel_vs_float64_reference(lib, n, n_steps):
    """B = 3 calls (the three seeds, the frames rotated so that every seed meets every frame) and a B = 1 call per (seed, frame): every row within
    2e-5 of the reference, padding untouched (ld = n + 3: rows 1 and 2 of a B = 3 call are not 16-byte aligned, row 0 and every B = 1 row are -
    both store forms), all (seed, frame, kind) rows pairwise different, a B = 3 row bit-identical to the B = 1 row of its seed and frame."""
    got3, got1, worst = {}, {}, 0.0
    for rot in range(3):
        frames = [FRAMES[(b + rot) % 3] for b in range(3)]
        rc, noise, sde = _call(lib, 3, n, n_steps, SEEDS, frames)
        assert rc == 0
        for b in range(3):
            for k, row in _rows(noise, sde, b, n, n_steps).items():
                got3[(SEEDS[b], frames[b], k)] = row
    for s in SEEDS:
        for f in FRAMES:
            rc, noise, sde = _call(lib, 1, n, n_steps, [s], [f])
            assert rc == 0
            for k, row in _rows(noise, sde, 0, n, n_steps).items():
                got1[(s, f, k)] = row
    assert set(got3) == set(got1) and len(got1) == 9 * (1 + n_steps)
    for key, row in got1.items():
        want = P.normal_row(*key, n)
        err = float(np.abs(row.astype(np.float64) - want).max())
        worst = max(worst, err)
        assert np.isfinite(row).all() and err <= BAR, (key, err)
        assert np.array_equal(row, got3[key]), key
    print(f"n {n}, n_steps {n_steps}: max abs error vs float64 reference {worst:.3e}")
    keys = sorted(got1)
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            assert not np.array_equal(got1[a], got1[b]), (a, b)


def test_noise_kernel_rejects_bad_arguments(lib):
    """every refusal of the header: a negative code, nothing launched - the buffers keep their sentinel"""
    n, n_steps, B = 8, 2, 2
    noise = torch.full((B, n), SENTINEL, device="cuda")
    sde = torch.full((B, n_steps * n), SENTINEL, device="cuda")
    sd, fr = _i64([1, 2]).cuda(), torch.zeros(B, dtype=torch.int32, device="cuda")
    good = dict(noise=noise.data_ptr(), ld_noise=n, sde=sde.data_ptr(), ld_sde=n_steps * n, B=B, n=n, n_steps=n_steps, seeds=sd.data_ptr(), frames=fr.data_ptr())
    bad = [dict(noise=None), dict(seeds=None), dict(frames=None), dict(B=0), dict(B=-1), dict(n=0), dict(n=-4), dict(n_steps=-1), dict(ld_noise=n - 1),
           dict(ld_sde=n_steps * n - 1)]
    for change in bad:
        a = dict(good, **change)
        rc = lib.vv_noise_normal(a["noise"], a["ld_noise"], a["sde"], a["ld_sde"], a["B"], a["n"], a["n_steps"], a["seeds"], a["frames"], None)
        assert rc < 0, (change, rc)
        assert lib.vv_last_error().decode().startswith("vv_noise_normal"), change
    torch.cuda.synchronize()
    assert bool((noise == SENTINEL).all()) and bool((sde == SENTINEL).all())
    # ld_sde is not looked at without sde_noise, and the good call goes through
    assert lib.vv_noise_normal(noise.data_ptr(), n, None, 0, B, n, n_steps, sd.data_ptr(), fr.data_ptr(), None) == 0
    assert lib.vv_noise_normal(*[good[k] for k in ("noise", "ld_noise", "sde", "ld_sde", "B", "n", "n_steps", "seeds", "frames")], None) == 0
    torch.cuda.synchronize()
    assert not bool((noise == SENTINEL).any()) and not bool((sde == SENTINEL).any())


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


def _kernel_rows(lib, seed, F, latent, n_steps):
    """what vv_noise_normal draws for frames 0 .. F - 1 of the dialogue with `seed`: (Z [F, latent], Zs [F, n_steps, latent]) on the CPU, read back from
    one call with B = F"""
    noise = torch.empty(F, latent, device="cuda")
    sde = torch.empty(F, max(n_steps, 1), latent, device="cuda")
    sd, fr = _i64([seed] * F).cuda(), torch.arange(F, dtype=torch.int32).cuda()
    rc = lib.vv_noise_normal(noise.data_ptr(), latent, sde.data_ptr(), max(n_steps, 1) * latent, F, latent, n_steps, sd.data_ptr(), fr.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return noise.cpu(), sde.cpu()[:, :n_steps]


def _same(a, b):
    assert a.sequences.tolist() == b.sequences.tolist()
    for x, y in zip(a.speech_outputs, b.speech_outputs):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.shape == y.shape and torch.equal(x, y)


def _sde_scheduler(sched):
    return sched.from_config(sched.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")


N_STEPS = 5
SEED1 = 0x5eed0123456789ab


def _tiny(use_graphs):
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg = VVConfig.preset("tiny")
    m = VibeVoiceForConditionalGenerationInference.from_synthetic(cfg, seed=1234, device="cuda:0", torch_dtype=torch.float32, use_graphs=use_graphs)
    m.set_ddpm_inference_steps(N_STEPS)
    return cfg, m


@pytest.mark.parametrize("use_graphs", [True, False])
def test_one_dialogue_device_noise_vs_injected_kernel_rows(lib, monkeypatch, use_graphs):
    """`tiny` fp32, forced SD SD SD SE ST SD SD SE EOS (with graphs the frames speculated at steps 3 and 7 are rolled back), ODE and SDE solver:
    device_noise=True, noise_seed=s is bit-identical - sequences and waveform - to the same call with the kernel's rows of frames 0 .. 4 injected as
    noise= (sde_noise=); with graphs, streaming through an AudioStreamer (graphs B1 / B2) is bit-identical to the non-streaming call."""
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.streamer import AudioStreamer
    cfg, m = _tiny(use_graphs)
    rollbacks = []
    real = Engine.rollback_speech_state
    monkeypatch.setattr(Engine, "rollback_speech_state", lambda self: (rollbacks.append(1), real(self))[1])
    try:
        tok = _Tok(cfg.vocab)
        D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
        forced = [D, D, D, E, S, D, D, E, EOS]
        F = forced.count(D)
        ids = _prompts(cfg, [24], 5)[0]
        kw = dict(input_ids=ids[None], tokenizer=tok, cfg_scale=1.3, forced_tokens=forced)
        ode = m.model.noise_scheduler
        for solver in ("ode", "sde"):
            if solver == "sde":
                m.model.noise_scheduler = _sde_scheduler(ode)
                m.set_ddpm_inference_steps(N_STEPS)
                assert m.engine.sde
            Z, Zs = _kernel_rows(lib, SEED1, F, cfg.latent, N_STEPS if solver == "sde" else 0)
            del rollbacks[:]
            dn = m.generate(device_noise=True, noise_seed=SEED1, **kw)
            assert len(rollbacks) == (2 if use_graphs else 0)
            inj = m.generate(noise=Z, sde_noise=Zs if solver == "sde" else None, **kw)
            assert dn.speech_outputs[0].shape == (1, F * cfg.hop) and bool(dn.speech_outputs[0].abs().max() > 0)
            _same(dn, inj)
            if use_graphs:
                st = AudioStreamer(batch_size=1, timeout=5)
                streamed = m.generate(device_noise=True, noise_seed=SEED1, audio_streamer=st, **kw)
                _same(streamed, dn)
                got = torch.cat([c.reshape(-1) for c in st.get_stream(0)])
                assert torch.equal(got, dn.speech_outputs[0][0].cpu())
                # the switch is part of the graph key: the injected call replayed the graph it replays without the feature
                assert {("B", 1.3, "dn"), ("B", 1.3), ("B1", 1.3, "dn")} <= set(m.engine._graphs) and ("B1", 1.3) not in m.engine._graphs
    finally:
        _drop(m)


def test_noise_seed_forms_and_refusals(lib):
    """The same noise_seed twice: bit-identical; another seed: another waveform; an explicit seed with greedy decoding leaves torch's CPU
    generator where it was; noise_seed=None draws the seed from that generator (two calls after the same manual_seed agree, and the state
    moves); device_noise with noise= and a seed list of the wrong length raise ValueError, as does noise_seed without device_noise."""
    cfg, m = _tiny(True)
    try:
        tok = _Tok(cfg.vocab)
        D, E, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id
        ids = _prompts(cfg, [24], 5)[0]
        kw = dict(input_ids=ids[None], tokenizer=tok, cfg_scale=1.3, forced_tokens=[D, D, D, E, EOS], device_noise=True)
        torch.manual_seed(11)
        state = torch.get_rng_state()
        a = m.generate(noise_seed=7, **kw)
        assert torch.equal(torch.get_rng_state(), state)
        b = m.generate(noise_seed=7, **kw)
        c = m.generate(noise_seed=8, **kw)
        lst = m.generate(noise_seed=[7], **kw)
        _same(a, b)
        _same(a, lst)
        assert not torch.equal(a.speech_outputs[0], c.speech_outputs[0])
        greedy = m.generate(input_ids=ids[None], tokenizer=tok, cfg_scale=1.3, max_new_tokens=6, device_noise=True, noise_seed=7)      # nothing forced
        assert torch.equal(torch.get_rng_state(), state) and greedy.sequences.shape[1] > 24
        torch.manual_seed(21)
        n1 = m.generate(**kw)
        moved = torch.get_rng_state()
        torch.manual_seed(21)
        n2 = m.generate(**kw)
        _same(n1, n2)
        torch.manual_seed(21)
        assert not torch.equal(torch.get_rng_state(), moved)
        with pytest.raises(ValueError):
            m.generate(noise=torch.zeros(3, cfg.latent), **kw)
        with pytest.raises(ValueError):
            m.generate(noise_seed=[1, 2], **kw)
        with pytest.raises(ValueError):
            m.generate(input_ids=ids[None], tokenizer=tok, forced_tokens=[D, EOS], noise_seed=3)
    finally:
        _drop(m)


# ---- batches: `mid` bf16 (the row-batched GEMVs do not take tiny's hidden 64) -------------------------------------------------------------
LENS = [30, 21, 26, 28, 23, 25]
SEEDS6 = [0x1111111111111111, 0xfedcba9876543210, 42, 2 ** 63 + 5, 7, 2 ** 64 - 1]


def _schedules(tok, B):
    """every dialogue in its steady state at steps 1 .. 3, then a turn switch (dialogue 0 of each three), an early end (1) and a longer run (2);
    chosen so that _BatchCoupling yields no replace / restart (asserted by the fixture): a dialogue is then the computation it is alone"""
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    three = [[D] * 4 + [E, S, D, D, E, EOS], [D] * 4 + [E, EOS], [D] * 4 + [E, S, D, D, D, EOS]]
    return [list(three[b % 3]) for b in range(B)]


def _batch_inputs(cfg, tok, B):
    prompts = _prompts(cfg, LENS[:B], 6)
    Lp = max(LENS[:B])
    ids = torch.stack([torch.cat([torch.full((Lp - n,), tok.pad_id), p]) for n, p in zip(LENS[:B], prompts)])
    mask = torch.stack([torch.cat([torch.zeros(Lp - n, dtype=torch.long), torch.ones(n, dtype=torch.long)]) for n in LENS[:B]])
    return prompts, ids, mask


@pytest.fixture(scope="module")
def mid(lib):
    """one `mid` bf16 model for the batched tests, and the lanes runs with device noise (3 and 6 dialogues) they all compare against"""
    from vibevoice_rocm_amd.batchloop import _BatchCoupling
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg = VVConfig.preset("mid")
    tok = _Tok(cfg.vocab)
    m = VibeVoiceForConditionalGenerationInference.from_synthetic(cfg, seed=1234, device="cuda:0", torch_dtype=torch.bfloat16)
    m.set_ddpm_inference_steps(N_STEPS)
    lanes = {}
    for B in (3, 6):
        sch = _schedules(tok, B)
        cp, fin = _BatchCoupling(B, tok.speech_start_id, tok.speech_diffusion_id), [False] * B
        for step in range(max(map(len, sch))):
            live = [b for b in range(B) if not fin[b]]
            toks = {b: sch[b][step] for b in live}
            assert cp.step(toks, [b for b in live if toks[b] != tok.eos_token_id]) == ([], [])
            for b in live:
                fin[b] = toks[b] == tok.eos_token_id
        _, ids, mask = _batch_inputs(cfg, tok, B)
        lanes[B] = m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=1.3, forced_tokens=sch, row_batch=False,
                              device_noise=True, noise_seed=SEEDS6[:B])
    yield cfg, tok, m, lanes
    _drop(m)


def test_lanes_device_noise_vs_injected_kernel_rows(lib, mid):
    """3 dialogues on the lanes with seeds [s0, s1, s2]: per dialogue bit-identical to the same lanes call with the kernel's rows injected as
    noise=[B, F, latent]"""
    cfg, tok, m, lanes = mid
    sch = _schedules(tok, 3)
    _, ids, mask = _batch_inputs(cfg, tok, 3)
    F = max(s.count(tok.speech_diffusion_id) for s in sch)
    Z = torch.stack([_kernel_rows(lib, SEEDS6[b], F, cfg.latent, 0)[0] for b in range(3)])
    inj = m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=1.3, forced_tokens=sch, row_batch=False, noise=Z)
    assert [o.shape[1] // cfg.hop for o in inj.speech_outputs] == [s.count(tok.speech_diffusion_id) for s in sch]
    _same(lanes[3], inj)
    assert not torch.equal(lanes[3].speech_outputs[0][:, : 4 * cfg.hop], lanes[3].speech_outputs[1][:, : 4 * cfg.hop])


@pytest.mark.parametrize("B", [3, 6])
def test_row_batch_speculates_with_device_noise_and_agrees_with_lanes(lib, mid, monkeypatch, B):
    """3 dialogues (one row batch) and 6 (two), forced schedules, nothing injected.  With device_noise the row-batched call speculates every live
    dialogue in the steady-state steps 1 .. 3 (a spy on _RowDriver.decode) and its waveforms agree with the lanes run with the same seeds to the
    bar of test_generate_row_batch_vs_lanes (rel RMS 1e-2); the same call without device_noise - drawn noise, today's path - speculates nobody."""
    from vibevoice_rocm_amd import modeling
    cfg, tok, m, lanes = mid
    sch = _schedules(tok, B)
    _, ids, mask = _batch_inputs(cfg, tok, B)
    seen = []
    real = modeling._RowDriver.decode

    def spy(self, live, forced, eligible, sample_fn, deliver, **k):
        toks, speculated = real(self, live, forced, eligible, sample_fn, deliver, **k)
        seen.append((list(live), set(speculated)))
        return toks, speculated
    monkeypatch.setattr(modeling._RowDriver, "decode", spy)
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=1.3, forced_tokens=sch, row_batch=True)
    out = m.generate(device_noise=True, noise_seed=SEEDS6[:B], **kw)
    with_dn = list(seen)
    del seen[:]
    torch.manual_seed(1)
    plain = m.generate(**kw)
    without = list(seen)
    assert len(with_dn) == len(without) == max(map(len, sch)) - 1
    assert all(spec == set(live) and len(live) == B for live, spec in with_dn[:3]), with_dn[:3]          # decode calls of steps 1, 2, 3
    assert all(spec == set() for _, spec in without), without
    assert out.sequences.tolist() == lanes[B].sequences.tolist() == plain.sequences.tolist()
    for b in range(B):
        a, r = out.speech_outputs[b], lanes[B].speech_outputs[b]
        assert a.shape == r.shape
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what=f"generate() {B} dialogues mid bf16 device_noise, row-batched vs lanes, dialogue {b}")
        print(f"B {B} dialogue {b}: waveform rel RMS row batch vs lanes {err:.3e}")
        assert err < 1e-2, (b, err)


def test_dialogue_sounds_the_same_alone_and_in_a_batch(lib, mid):
    """dialogue 1 of the 3-dialogue lanes call against a single-dialogue call with noise_seed=s1 on its (unpadded) prompt and schedule: bit-identical"""
    cfg, tok, m, lanes = mid
    sch = _schedules(tok, 3)
    prompts, ids, _ = _batch_inputs(cfg, tok, 3)
    alone = m.generate(input_ids=prompts[1][None], tokenizer=tok, cfg_scale=1.3, forced_tokens=sch[1], device_noise=True, noise_seed=SEEDS6[1])
    Lp = ids.shape[1]
    assert alone.sequences[0, LENS[1]:].tolist() == lanes[3].sequences[1, Lp: Lp + len(sch[1])].tolist() == sch[1]
    assert torch.equal(alone.speech_outputs[0], lanes[3].speech_outputs[1])


def test_row_batch_sde_solver_device_noise_agrees_with_lanes(lib, mid):
    """The SDE solver on the row batch (graph H draws the variance noise of all steps too): 3 dialogues, nothing injected, against the lanes with
    the same seeds - the lanes' SDE form is pinned bit for bit by the one-dialogue test - at the row-batch-vs-lanes bar of
    test_generate_sde_row_batch_vs_lanes (1e-2); the waveforms differ from the ODE solver's."""
    cfg, tok, m, lanes = mid
    sch = _schedules(tok, 3)
    _, ids, mask = _batch_inputs(cfg, tok, 3)
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=1.3, forced_tokens=sch, device_noise=True, noise_seed=SEEDS6[:3])
    ode = m.model.noise_scheduler
    m.model.noise_scheduler = _sde_scheduler(ode)
    m.set_ddpm_inference_steps(N_STEPS)
    try:
        assert m.engine.sde
        ref = m.generate(row_batch=False, **kw)
        out = m.generate(row_batch=True, **kw)
        assert m._rowbatch[(3, 0)].sde and ("H", 1.3, "dn") in m._rowbatch[(3, 0)]._graphs
    finally:
        m.model.noise_scheduler = ode
        m.set_ddpm_inference_steps(N_STEPS)
    assert out.sequences.tolist() == ref.sequences.tolist()
    for b in range(3):
        a, r = out.speech_outputs[b], ref.speech_outputs[b]
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what=f"generate() 3 dialogues mid bf16 device_noise SDE, row-batched vs lanes, dialogue {b}")
        print(f"SDE dialogue {b}: waveform rel RMS row batch vs lanes {err:.3e}")
        assert a.shape == r.shape and err < 1e-2, (b, err)
        assert not torch.equal(r, lanes[3].speech_outputs[b])


def test_device_noise_with_device_sampling_keeps_tokens_and_generator_state(lib):
    """do_sample on `tiny` fp32, nothing forced, device_noise with an explicit seed: device_sampling=True against the host sampler of the same
    seeded call.  The noise no longer comes from the CPU generator, so there is nothing to rewind after a mis-speculated frame: same tokens,
    same torch.get_rng_state() afterwards, waveforms at the bar of test_generate_single_dialogue_device_sampling_vs_host_sampler (1e-2: the
    two forms of graph A normalise the hidden row in different kernels), and the call samples at least one frame."""
    cfg, m = _tiny(True)
    try:
        tok = _Tok(cfg.vocab)
        ids = _prompts(cfg, [24], 5)[0]
        gen_cfg = {"do_sample": True, "temperature": 1.0, "top_p": 0.95}
        res = {}
        for dev in (False, True):
            torch.manual_seed(0)
            out = m.generate(input_ids=ids[None], tokenizer=tok, cfg_scale=1.3, generation_config=gen_cfg, max_new_tokens=24, device_sampling=dev,
                             device_noise=True, noise_seed=SEED1)
            res[dev] = (out, torch.get_rng_state())
    finally:
        _drop(m)
    (oh, sh), (od, sd_) = res[False], res[True]
    print("sampled tokens:", od.sequences[0, 24:].tolist())
    assert od.sequences.tolist() == oh.sequences.tolist() and torch.equal(sd_, sh)
    assert tok.speech_diffusion_id in od.sequences[0, 24:].tolist()
    err = rel_rms(od.speech_outputs[0].float().cpu().numpy(), oh.speech_outputs[0].float().cpu().numpy(),
                  what="generate() tiny fp32 do_sample + device_noise, device sampler vs host sampler")
    print(f"waveform rel RMS device vs host sampler with device noise: {err:.3e}")
    assert err < 1e-2, err
