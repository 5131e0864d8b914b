"""The CPU oracle (oracle/vv_oracle.py) against fixtures captured from the reference's own modules
(oracle/gen/make_golden.py).  CPU only.  Tolerances: fp32, different summation order only."""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_rms
from oracle import vv_oracle as O

TOL = 2e-5


def t(x):
    return torch.from_numpy(np.asarray(x))


def test_scheduler_tables_and_trajectory():
    g = load_golden("scheduler")
    ac = O.cosine_alphas_cumprod(1000)
    np.testing.assert_allclose(ac.numpy(), g["alphas_cumprod"], rtol=0, atol=0)
    for n in (10, 20, 50):
        ts, sig = O.dpm_set_timesteps(ac, n)
        assert ts.tolist() == g[f"timesteps_{n}"].tolist()
        np.testing.assert_array_equal(sig.numpy(), g[f"sigmas_{n}"])
    # known answers quoted in SURVEY.md §8a row 4
    ts, sig = O.dpm_set_timesteps(ac, 20)
    assert ts[:3].tolist() == [999, 949, 899] and ts[-1] == 50
    assert abs(float(sig[1]) - 12.807271) < 1e-5 and float(sig[-1]) == 0.0
    for n in (10, 20):
        _, coefs = O.make_dpm_tables(dict(ddpm_steps=1000), n)
        assert [c["order"] for c in coefs] == [1] + [2] * (n - 2) + [1]
        x = t(g[f"traj_x0_{n}"])
        m_prev = None
        for i in range(n):
            x, m_prev = O.dpm_step(coefs[i], x, 0.1 * x, m_prev)
            assert rel_rms(x.numpy(), g[f"traj_{n}"][i]) < 1e-5, (n, i)


def test_head_forward(tiny_cfg, tiny_weights):
    g = load_golden("head_tiny")
    cfg = tiny_cfg.as_dict()
    for tt in (999, 500, 50):
        out = O.head_forward(tiny_weights, cfg, t(g["x"]), torch.full((3,), float(tt)), t(g["cond"]))
        assert rel_rms(out.numpy(), g[f"out_t{tt}"]) < TOL


def test_sample_speech_tokens(tiny_cfg, tiny_weights):
    g = load_golden("sample_tiny")
    cfg = tiny_cfg.as_dict()
    for n in (10, 20):
        for cs in (1.0, 1.3, 2.0):
            lat = O.sample_speech_tokens(tiny_weights, cfg, t(g["cond"]), t(g["ncond"]), t(g["noise"]), cs, n)
            assert rel_rms(lat.numpy(), g[f"latent_n{n}_cfg{cs}"]) < 1e-4, (n, cs)


def test_sample_speech_tokens_sde_solver(tiny_cfg, tiny_weights):
    """The SDE solver main.py selects (scheduler.from_config(algorithm_type="sde-dpmsolver++"), main.py:543-548): the reference's own
    sample_speech_tokens with the per-step variance noise replayed from the seeded CPU generator."""
    g = load_golden("sample_sde_tiny")
    cfg = tiny_cfg.as_dict()
    for n in (10, 20):
        lat = O.sample_speech_tokens(tiny_weights, cfg, t(g["cond"]), t(g["ncond"]), t(g["noise"]), 1.5, n, algorithm="sde-dpmsolver++",
                                     sde_noise=t(g[f"step_noise_n{n}"]))
        assert rel_rms(lat.numpy(), g[f"latent_n{n}"]) < 1e-4, n
        ode = O.sample_speech_tokens(tiny_weights, cfg, t(g["cond"]), t(g["ncond"]), t(g["noise"]), 1.5, n)
        assert rel_rms(ode.numpy(), g[f"latent_n{n}"]) > 1e-2          # and it is not the ODE solver's answer


def test_decoder_streaming_and_full(tiny_cfg, tiny_weights):
    g = load_golden("decoder_tiny")
    cfg = tiny_cfg.as_dict()
    st = O.ConvState()
    for f in range(g["latents"].shape[0]):
        if f == int(g["reset_before"]):
            st.zero()
        wav = O.tokenizer_decoder(tiny_weights, cfg, t(g["latents"][f])[:, None], st)
        assert wav.shape == (1, tiny_cfg.hop)
        assert rel_rms(wav[0].numpy(), g["wav_stream"][f]) < TOL, f
    full = O.tokenizer_decoder(tiny_weights, cfg, t(g["latents"][:5]).t(), None)
    assert rel_rms(full[0].numpy(), g["wav_full5"]) < TOL
    # the invariant the reference itself satisfies: streaming == non-streaming
    assert rel_rms(g["wav_stream"][:5].reshape(-1), g["wav_full5"]) < 1e-5


def test_semantic_streaming_full_and_ragged_acoustic(tiny_cfg, tiny_weights):
    g = load_golden("semantic_tiny")
    cfg = tiny_cfg.as_dict()
    st = O.ConvState()
    for f in range(g["wav"].shape[0]):
        if f == int(g["reset_before"]):
            st.zero()
        feat = O.semantic_encode(tiny_weights, cfg, t(g["wav"][f])[None], st)
        assert rel_rms(feat[0].numpy(), g["feat_stream"][f]) < TOL, f
    full = O.semantic_encode(tiny_weights, cfg, t(g["wav"][:4].reshape(1, -1)), None)
    assert rel_rms(full.numpy(), g["feat_full4"]) < TOL
    ac = O.acoustic_encode(tiny_weights, cfg, t(g["ragged_wav"])[None])
    assert ac.shape == g["ragged_acoustic_mean"].shape
    assert rel_rms(ac.numpy(), g["ragged_acoustic_mean"]) < TOL


def test_connectors(tiny_weights):
    g = load_golden("connector_tiny")
    assert rel_rms(O.connector(tiny_weights, "model.acoustic_connector.", t(g["a"])).numpy(), g["a_out"]) < TOL
    assert rel_rms(O.connector(tiny_weights, "model.semantic_connector.", t(g["s"])).numpy(), g["s_out"]) < TOL


def test_llm_prefill_and_decode(tiny_cfg, tiny_weights):
    g = load_golden("llm_tiny")
    cfg = tiny_cfg.as_dict()
    emb = tiny_weights["model.language_model.embed_tokens.weight"]
    kv = O.KVCache(tiny_cfg.layers)
    h = O.llm_forward(tiny_weights, cfg, emb[t(g["ids"])], kv, 0)
    assert rel_rms(h.numpy(), g["prefill_hidden"]) < TOL
    logits = h[-1] @ O.lm_head_weight(tiny_weights, cfg).t()
    assert rel_rms(logits.numpy(), g["prefill_logits"]) < TOL
    for i in range(3):
        h = O.llm_forward(tiny_weights, cfg, t(g["decode_embeds"][i])[None], kv, kv.length)
        assert rel_rms(h[0].numpy(), g["decode_hidden"][i]) < TOL, i
    assert rel_rms(kv.k[0].numpy(), g["k_cache_l0"]) < TOL
    assert rel_rms(kv.v[1].numpy(), g["v_cache_l1"]) < TOL


def test_process_speech_inputs(tiny_cfg, tiny_weights):
    g = load_golden("speech_inputs_tiny")
    feats, conn = O.process_speech_inputs(tiny_weights, tiny_cfg.as_dict(), t(g["wav"]), t(g["masks"]),
                                          t(g["std_noise"]), t(g["eps_noise"]))
    assert rel_rms(feats.numpy(), g["feats"]) < TOL
    assert rel_rms(conn.numpy(), g["connected"]) < TOL


def test_generate_loop_trace(tiny_cfg, tiny_weights):
    """The loop restatement against the hand-driven reference trace, which performs the reference's own
    negative-branch attention-mask / KV surgery: pins 'reset == truncate to empty context'."""
    g = load_golden("loop_trace_tiny")
    cfg = tiny_cfg.as_dict()
    ST, E, D, EOS = [int(v) for v in g["special"]]
    special = dict(speech_start=ST, speech_end=E, speech_diffusion=D, eos=EOS)
    _, conn = O.process_speech_inputs(tiny_weights, cfg, t(g["voice"]), t(g["speech_masks"]), t(g["std_noise"]), t(g["eps_noise"]))
    res = O.generate(tiny_weights, cfg, g["ids"].tolist(), t(g["speech_input_mask"]), conn, special, t(g["noise"]),
                     cfg_scale=float(g["cfg_scale"]), n_steps=int(g["n_steps"]), forced_tokens=g["forced"].tolist(),
                     keep_trace=True)
    assert res.sequences[len(g["ids"]):] == g["tokens"].tolist()
    frames = [r for r in res.trace if "latent" in r]
    assert len(frames) == g["latent"].shape[0] == 5
    for i, r in enumerate(frames):
        assert rel_rms(r["cond"].numpy(), g["cond"][i]) < 1e-4, i
        assert rel_rms(r["ncond"].numpy(), g["ncond"][i]) < 1e-4, i
        assert rel_rms(r["latent"].numpy(), g["latent"][i]) < 2e-4, i
        assert rel_rms(r["wav"].numpy(), g["wav"][i]) < 5e-4, i
        assert rel_rms(r["sem"].numpy(), g["sem"][i]) < 5e-4, i
    for i in range(g["next_embeds"].shape[0]):
        assert rel_rms(res.trace[i]["next_embeds"].numpy(), g["next_embeds"][i]) < 5e-4, i


@pytest.mark.parametrize("preset", ["tiny", "mid"])
def test_oracle_vs_reference_bf16_run(preset):
    """tests/golden/sample_bf16_*.npz: the reference's head / sample_speech_tokens run in bf16 on the CPU, and the same model in fp32
    on the same bf16-representable weights.  (1) the fp32 run pins the oracle once more (a second weight set, 10 and 20 steps);
    (2) the oracle's `bf16_t` option - t cast to bf16 before the sinusoid, the sinusoid cast back (modeling_vibevoice_inference.py:703,
    modular_vibevoice_diffusion_head.py:88) - is what moves fp32 arithmetic onto the reference's bf16 results; what remains is the
    reference's own bf16 rounding noise, which calibrates the bf16 tolerance of the GPU tests (measured here: 6e-3 .. 1e-2)."""
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset(preset)
    sd = {k: torch.from_numpy(v).to(torch.bfloat16).float() for k, v in synth_state_dict(cfg, 1234).items()}
    g = load_golden(f"sample_bf16_{preset}")
    c, nc, noise = (torch.from_numpy(g[k]) for k in ("cond", "ncond", "noise"))
    x, c3 = torch.from_numpy(g["x"]), torch.from_numpy(g["cond3"])
    for t in (999, 500, 50):
        tt = torch.full((3,), float(t))
        e32 = rel_rms(O.head_forward(sd, cfg.as_dict(), x, tt, c3).numpy(), g[f"head_fp32_t{t}"])
        eq = rel_rms(O.head_forward(sd, cfg.as_dict(), x, tt, c3, bf16_t=True).numpy(), g[f"head_bf16_t{t}"])
        floor = rel_rms(g[f"head_fp32_t{t}"], g[f"head_bf16_t{t}"])
        assert e32 < 2e-6, f"head t={t}: oracle vs reference fp32 {e32:.3e}"
        assert eq < 1.2e-2, f"head t={t}: oracle(bf16_t) vs reference bf16 {eq:.3e} (reference fp32 vs bf16 {floor:.3e})"
    # t = 999 rounds to 1000 in bf16: without the rounding the fp32 arithmetic is several times further from the bf16 run
    assert rel_rms(g["head_fp32_t999"], g["head_bf16_t999"]) > 3 * rel_rms(
        O.head_forward(sd, cfg.as_dict(), x, torch.full((3,), 999.0), c3, bf16_t=True).numpy(), g["head_bf16_t999"])
    for n in (10, 20):
        for cs in (1.3, 2.0):
            e32 = rel_rms(O.sample_speech_tokens(sd, cfg.as_dict(), c, nc, noise, cs, n).numpy(), g[f"latent_fp32_n{n}_cfg{cs}"])
            eq = rel_rms(O.sample_speech_tokens(sd, cfg.as_dict(), c, nc, noise, cs, n, bf16_t=True).numpy(), g[f"latent_bf16_n{n}_cfg{cs}"])
            assert e32 < 2e-6, f"n={n} cfg={cs}: oracle vs reference fp32 {e32:.3e}"
            assert eq < 1.5e-2, f"n={n} cfg={cs}: oracle(bf16_t) vs reference bf16 {eq:.3e}"


def test_oracle_vs_reference_components_fp32_and_bf16_floor():
    """tests/golden/components_bf16_mid.npz: the reference's streaming acoustic decoder, streaming semantic encoder and Qwen2 prefill +
    cached decode steps at `mid` shapes (head_dim 128, GQA) on bf16-representable weights, run in fp32 and in bf16.  (1) the fp32 legs pin
    the oracle on a second weight set and on the `mid` shapes the GPU tests use; (2) |bf16 run - fp32 run| is the reference's own bf16
    noise floor per component - the GPU tests' bf16 bars are stated as multiples of it, so it is asserted to sit where it was measured
    (8.6e-3 .. 9.2e-3): a regenerated fixture that moves it moves the bars knowingly."""
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("mid")
    ocfg = cfg.as_dict()
    sd = {k: torch.from_numpy(v).to(torch.bfloat16).float() for k, v in synth_state_dict(cfg, 1234).items()}
    g = load_golden("components_bf16_mid")
    st_d, st_s = O.ConvState(), O.ConvState()
    for f in range(3):
        wav = O.tokenizer_decoder(sd, ocfg, torch.from_numpy(g["latents"][f])[:, None], st_d)[0]
        sem = O.semantic_encode(sd, ocfg, torch.from_numpy(g["wav_in"][f])[None], st_s)[0]
        ed, es = rel_rms(wav.numpy(), g["wav_fp32"][f]), rel_rms(sem.numpy(), g["sem_fp32"][f])
        assert ed < 2e-5 and es < 2e-5, f"frame {f}: oracle vs reference fp32: decoder {ed:.3e} semantic {es:.3e}"
    emb = sd["model.language_model.embed_tokens.weight"]
    kv = O.KVCache(cfg.layers)
    h = O.llm_forward(sd, ocfg, emb[torch.from_numpy(g["ids"])], kv, 0)[-1]
    e = rel_rms(h.numpy(), g["prefill_hidden_fp32"])
    assert e < 2e-5, f"oracle vs reference fp32 prefill: {e:.3e}"
    for i in range(2):
        h = O.llm_forward(sd, ocfg, torch.from_numpy(g["decode_embeds"][i])[None], kv, kv.length)[0]
        e = rel_rms(h.numpy(), g["decode_hidden_fp32"][i])
        assert e < 2e-5, f"oracle vs reference fp32 decode step {i}: {e:.3e}"
    for key in ("wav", "sem", "prefill_hidden", "decode_hidden"):
        floor = rel_rms(g[key + "_bf16"], g[key + "_fp32"])
        assert 6e-3 < floor < 1.2e-2, f"{key}: reference bf16 vs fp32 floor {floor:.3e}"


def _batch_trace_inputs(g, entry, b, cfg, W):
    """sample b of a loop_trace_batch entry, unpadded, with its own voice prompt encoded through the oracle"""
    keep = g[f"{entry}_attention_mask"][b].astype(bool)
    _, conn = O.process_speech_inputs(W, cfg, t(g[f"{entry}_voice"][b:b + 1]), t(g[f"{entry}_speech_masks"][b:b + 1]),
                                      t(g[f"{entry}_std_noise"][b:b + 1]), t(g[f"{entry}_eps_noise"][b:b + 1]))
    return g[f"{entry}_ids"][b][keep].tolist(), t(g[f"{entry}_speech_input_mask"][b][keep]), conn


@pytest.mark.parametrize("preset", ["tiny", "mid"])
def test_generate_loop_trace_batch(preset):
    """tests/golden/loop_trace_batch_*.npz: the reference's BATCHED loop, hand-driven with its own negative-branch mask / KV surgery and its
    own streaming tokenizer cache for all samples at once, left-padded prompts of different lengths, one voice prompt per sample.  Every
    sample against a per-sample oracle run.  Entry a (interleaved segments, an early EOS, a speech_start while another sample diffuses)
    needs no batch rule; entry b trips the guard disagreement of :595 / :607 (batch_negative_replacements), entry c the streaming cache's
    all-or-nothing get() (batch_conv_restarts).  For b and c the plain per-sample run is checked to DIFFER from the fixture, so the rules
    are needed, not decoration."""
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    vc = VVConfig.preset(preset)
    g = load_golden(f"loop_trace_batch_{preset}")
    cfg = vc.as_dict()
    W = {k: torch.from_numpy(v) for k, v in synth_state_dict(vc, 1234).items()}
    if int(g["weights_bf16"]):
        W = {k: (v.to(torch.bfloat16).float() if v.dim() >= 1 else v) for k, v in W.items()}
    ST, E, D, EOS = [int(v) for v in g["special"]]
    special = dict(speech_start=ST, speech_end=E, speech_diffusion=D, eos=EOS)
    valid = sorted([ST, E, D, EOS])
    lm = O.lm_head_weight(W, cfg)[valid].double()
    for entry, n_repl, n_restart in (("a", 0, 0), ("b", 1, 0), ("c", 0, 1)):
        B = g[f"{entry}_ids"].shape[0]
        forced = [g[f"{entry}_s{b}_forced"].tolist() for b in range(B)]
        repl = O.batch_negative_replacements(forced, special)
        rest = O.batch_conv_restarts(forced, special)
        assert sum(len(r) for r in repl) == n_repl and sum(len(r) for r in rest) == n_restart, (entry, repl, rest)
        assert int(g[f"{entry}_n_guard"]) > 0 or not n_repl        # a replacement needs a guard disagreement (a has harmless ones)
        for b in range(B):
            ids, sp, conn = _batch_trace_inputs(g, entry, b, cfg, W)
            runs = [(repl[b], rest[b])] + ([(set(), set())] if (repl[b] or rest[b]) else [])
            for k, (rs, cs) in enumerate(runs):
                res = O.generate(W, cfg, ids, sp, conn, special, t(g[f"{entry}_s{b}_noise"]), cfg_scale=float(g["cfg_scale"]),
                                 n_steps=int(g["n_steps"]), forced_tokens=forced[b], keep_trace=True, neg_replace_steps=rs, conv_restart_steps=cs)
                assert res.sequences[len(ids):] == g[f"{entry}_s{b}_tokens"].tolist()
                frames = [r for r in res.trace if "latent" in r]
                assert len(frames) == g[f"{entry}_s{b}_latent"].shape[0]
                e_wav = rel_rms(torch.cat(res.audio).numpy(), g[f"{entry}_s{b}_wav"].reshape(-1))
                if k == 1:
                    assert e_wav > 1e-2, f"{entry} sample {b}: the per-sample semantics alone already match ({e_wav:.2e})"
                    continue
                for i, r in enumerate(frames):
                    assert rel_rms(r["cond"].numpy(), g[f"{entry}_s{b}_cond"][i]) < 1e-4, (entry, b, i)
                    assert rel_rms(r["ncond"].numpy(), g[f"{entry}_s{b}_ncond"][i]) < 1e-4, (entry, b, i)
                    assert rel_rms(r["latent"].numpy(), g[f"{entry}_s{b}_latent"][i]) < 2e-4, (entry, b, i)
                    assert rel_rms(r["wav"].numpy(), g[f"{entry}_s{b}_wav"][i]) < 5e-4, (entry, b, i)
                assert e_wav < 5e-4, (entry, b, e_wav)
