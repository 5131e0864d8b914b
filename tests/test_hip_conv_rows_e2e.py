"""generate() and a serving session with batched_conv_rows=True (the one-row stage of both tokenizers and the connectors once per row batch,
rowbatch.RowBatch.enable_conv_rows) on the 1.5B preset, against the lanes and against each dialogue alone.  The schedules are those of
tests/test_hip_rowbatch_wide.py::_dialogues - an early end and a rolled-back speculated frame among them - and every bar is the one the
row-batch-vs-lanes tests hold (same sequences, waveform relative RMS < 1e-2)."""
import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

BAR = 1e-2


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
    assert m.batched_conv_rows is False          # off by default
    m.set_ddpm_inference_steps(20)
    return cfg, sd, m


def _same(got, want, B, what):
    assert got.sequences.tolist() == want.sequences.tolist()
    for b in range(B):
        assert got.speech_outputs[b].shape == want.speech_outputs[b].shape
        err = rel_rms(got.speech_outputs[b].float().cpu().numpy(), want.speech_outputs[b].float().cpu().numpy(), what=f"{what}, waveform of dialogue {b}")
        print(f"{what}, dialogue {b}: waveform rel RMS {err:.3e}")
        assert err < BAR, f"{what}, dialogue {b}: waveform rel RMS {err:.3e}"


@pytest.mark.parametrize("B, width, keys", [(3, 4, [(3, 0)]), (6, 4, [(3, 0, "side"), (3, 3, "side")]), (6, 8, [(6, 0, "side")])])
def test_generate_batched_conv_rows_vs_lanes(big, B, width, keys):
    from test_hip_rowbatch_wide import _dialogues
    cfg, sd, m = big
    tok, kw = _dialogues(cfg, B, 37 + B)
    rows = m.generate(row_batch=True, row_batch_width=width, batched_conv_rows=True, **kw)
    assert all(k + ("conv_rows",) in m._rowbatch for k in keys), sorted(map(str, m._rowbatch))
    for k in keys:
        rb = m._rowbatch[k + ("conv_rows",)]
        assert rb.conv_rows is not None and rb.conv_rows.owed == set()
        kinds = [kind for kind, _ in rb.conv_rows.log]
        assert "front" in kinds and "back" in kinds
        assert ("front",) in rb._graphs and ("back",) in rb._graphs and not any(g[0] == "RBconv" for e in rb.lanes for g in e._graphs if g[-1] == rb.uid)
    lanes = m.generate(row_batch=False, **kw)
    _same(rows, lanes, B, f"generate(batched_conv_rows=True) on {B} dialogues (width {width}) 1.5B bf16 vs lanes")
    # a default call in the same process: today's keys, today's per-dialogue tails, the lanes' result
    plain = m.generate(row_batch=True, row_batch_width=width, **kw)
    for k in keys:
        assert k in m._rowbatch and m._rowbatch[k].conv_rows is None
        assert ("front",) not in m._rowbatch[k]._graphs
    _same(plain, lanes, B, f"default generate() on {B} dialogues (width {width}) after a batched_conv_rows call vs lanes")


def test_generate_batched_conv_rows_with_device_noise_speculates(big, monkeypatch):
    """3 dialogues, device_noise=True, nothing injected: every live dialogue is speculated in the steady-state steps (the spy of
    tests/test_hip_device_noise.py), so a step's front serves all of them and the rolled-back frame of dialogue 1 owes no back"""
    from test_hip_rowbatch_wide import _dialogues
    from vibevoice_rocm_amd import modeling
    cfg, sd, m = big
    B = 3
    tok, kw = _dialogues(cfg, B, 51)
    kw.pop("noise")
    seeds = [4100 + b for b in range(B)]
    seen = []
    real = modeling._RowDriver.decode

    def spy(self, live, forced, eligible, sample_fn, deliver, **k):
        toks, speculated = real(self, live, forced, eligible, sample_fn, deliver, **k)
        seen.append((list(live), set(speculated)))
        return toks, speculated
    monkeypatch.setattr(modeling._RowDriver, "decode", spy)
    rows = m.generate(row_batch=True, batched_conv_rows=True, device_noise=True, noise_seed=seeds, **kw)
    # decode calls of steps 1 and 2: all three are in their steady state (dialogue 0's second speculated frame is then rolled back)
    assert all(spec == set(live) and len(live) == B for live, spec in seen[:2]), seen[:2]
    monkeypatch.setattr(modeling._RowDriver, "decode", real)
    lanes = m.generate(row_batch=False, device_noise=True, noise_seed=seeds, **kw)
    _same(rows, lanes, B, "generate(batched_conv_rows=True, device_noise=True) on 3 dialogues 1.5B bf16 vs lanes with the same seeds")


def test_session_with_batched_conv_rows(big):
    """A 4-slot session on a model with the flag on serves 6 ragged requests, so slots are refilled; each against generate() on it alone"""
    cfg, sd, m = big
    from test_hip_rowbatch_wide import _Tok
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(67)
    lens = [50, 37, 44, 29, 41, 33]
    n = len(lens)
    prompts = [torch.cat([torch.randint(0, 1000, (k - 1,), generator=g), torch.tensor([S])]) for k in lens]
    forced = [[D] * (2 + (3 * i) % 5) + ([E, S, D, D] if i == 2 else []) + [E, EOS] for i in range(n)]
    noise = torch.randn(n, 8, cfg.latent, generator=g)
    scales = [1.3, 2.0, 3.0, 2.0, 1.3, 3.0]
    m.batched_conv_rows = True          # open_session inherits the model's value
    try:
        with m.open_session(tokenizer=tok, slots=4, max_context=256, device_noise=False) as sess:
            assert (4, 0, "session", "conv_rows") in m._rowbatch and m._rowbatch[(4, 0, "session", "conv_rows")].conv_rows is not None
            hs = [sess.submit(input_ids=prompts[i][None], cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i]) for i in range(n)]
            sess.run()
            got = [h.result() for h in hs]
            assert len({h.slot for h in hs}) < n          # a slot served more than one request
    finally:
        m.batched_conv_rows = False
    for i in range(n):
        want = m.generate(input_ids=prompts[i][None], tokenizer=tok, cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i])
        assert got[i].sequences.tolist() == want.sequences.tolist(), i
        err = rel_rms(got[i].speech_outputs[0].float().cpu().numpy(), want.speech_outputs[0].float().cpu().numpy(),
                      what=f"session of 4 slots with batched_conv_rows, request {i} vs generate() alone")
        print(f"session request {i}: waveform rel RMS {err:.3e}")
        assert err < BAR, f"request {i}: waveform rel RMS {err:.3e}"
