"""Voice prefix cache on the GPU: model.prepare_voice_prefix + generate(voice_prefix=...) against the full-prompt generate() of the same
prompt, voices, forced tokens and injected noise.

The two paths compute the same function (attention is causal: the prefix positions' K / V do not depend on the script); what differs is how
many rows each prefill GEMM sees, i.e. the tiling of the bf16 / fp32 products - the situation of "same prompt, different prefill chunking",
whose bars the project already has:
  bf16   2e-2 waveform rel RMS   (test_hip_round3.py::test_cfg5_end_to_end_7b_fp8_50_steps_chunked_prefill_streamer, chunked vs one chunk)
  fp32   1e-3 waveform rel RMS   (test_hip_parity.py::test_generate_loop_vs_reference_trace, the fp32 loop trace at `tiny`)
  fp8 KV the weight-only-fp8 deviation measured on the same call (test_hip_kv_fp8.py::test_fp8_kv_deviation_against_the_accepted_lossy_mode)
  lanes vs single calls: bit-identical (test_hip_kv_fp8.py / test_hip_nf4.py); row batch vs lanes: 1e-2 (test_hip_rowbatch.py::test_generate_row_batch_vs_lanes)

Prompt: 60 prefix tokens (text, one 3-frame voice, text) + 25 script tokens ending in speech_start; 3 forced frames."""
import numpy as np
import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

P_LEN, SUFFIX = 60, 25


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class _Tok:
    def __init__(self, v):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = v - 4, v - 3, v - 2, v - 1
        self.bos_token_id = None
        self.pad_id = 0


def _inputs(cfg, seed=17, suffixes=(SUFFIX,)):
    """prefix ids / mask / voice / injected voice noise, one suffix per entry of `suffixes`, forced tokens (3 frames) and diffusion noise"""
    V = cfg.vocab
    ST, SE, SD, EOS = V - 4, V - 3, V - 2, V - 1
    g = torch.Generator().manual_seed(seed)
    pre = torch.randint(1, V - 8, (40,), generator=g).tolist() + [7, ST, SD, SD, SD, SE, 9] + torch.randint(1, V - 8, (13,), generator=g).tolist()
    mask = [False] * 42 + [True] * 3 + [False] * 15
    assert len(pre) == len(mask) == P_LEN
    d = dict(V=V, tok=_Tok(V), pre=torch.tensor(pre), pre_mask=torch.tensor(mask), wav=0.1 * torch.randn(1, 3 * cfg.hop - 321, generator=g),
             sm=torch.ones(1, 3, dtype=torch.bool), speech_noise=(torch.randn(1, generator=g), torch.randn(1, 3, cfg.ac_dim, generator=g)))
    d["suffix"] = [torch.cat([torch.randint(1, V - 8, (n - 1,), generator=g), torch.tensor([ST])]) for n in suffixes]
    d["forced"] = [[SD, SD, SD, SE, EOS], [SD, SD, SE, EOS], [SD, SE, ST, SD, SD, SE, EOS]][: len(suffixes)]
    d["noise"] = torch.randn(len(suffixes), 4, cfg.latent, generator=g)
    return d


def _prepare(m, d):
    return m.prepare_voice_prefix(d["pre"], d["wav"], d["sm"], d["pre_mask"], speech_noise=d["speech_noise"])


def _single(m, d, b=0, vp=None, **kw):
    """one dialogue: with vp the prefix path (no voice tensors handed over), without it the full prompt"""
    ids = torch.cat([d["pre"], d["suffix"][b]])
    mask = torch.cat([d["pre_mask"], torch.zeros(len(d["suffix"][b]), dtype=torch.bool)])
    args = dict(input_ids=ids[None], speech_input_mask=mask[None], tokenizer=d["tok"], cfg_scale=2.0, forced_tokens=d["forced"][b], noise=d["noise"][b])
    if vp is None:
        args.update(speech_tensors=d["wav"], speech_masks=d["sm"], speech_noise=d["speech_noise"])
    else:
        args.update(voice_prefix=vp)
    args.update(kw)
    return m.generate(**args)


def _wav(out, b=0):
    return out.speech_outputs[b][0].float().cpu().numpy()


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset("mid")
    sd = synth_state_dict_torch(cfg, 4242, device="cuda:0", dtype=torch.bfloat16)
    models = {}

    def get(name):
        if name not in models:
            kw = dict(bf16={}, kv8=dict(kv_cache_dtype="fp8"), w8=dict(weight_quant="fp8"), nf4=dict(weight_quant="nf4"))[name]
            models[name] = M(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, **kw)
            models[name].set_ddpm_inference_steps(10)
        return models[name]
    yield cfg, get
    for m in models.values():
        m.release_lanes()
        m.engine.close()


@pytest.fixture(scope="module")
def bf16_case(mid):
    """the bf16 model, its inputs, the prepared prefix and the full-prompt reference run (computed once, shared, never modified)"""
    cfg, get = mid
    m = get("bf16")
    d = _inputs(cfg)
    full = _single(m, d)
    vp = _prepare(m, d)
    return m, d, vp, full


def test_store_layout(bf16_case, mid):
    cfg, _ = mid
    m, d, vp, _ = bf16_case
    assert vp.P == P_LEN and vp.ids.tolist() == d["pre"].tolist()
    assert tuple(vp.k.shape) == tuple(vp.v.shape) == (cfg.layers, 1, cfg.kv_heads, 64, cfg.head_dim) and vp.k.dtype == torch.bfloat16
    assert vp.kv.rows == 1 and vp.kv.s_max == 64 and not vp.kv.vt and vp.nbytes == 2 * vp.k.numel() * 2
    k = vp.k.float()
    assert bool(torch.isfinite(k).all()) and float(k[:, :, :, :P_LEN].abs().max()) > 0 and float(k[:, :, :, P_LEN:].abs().max()) == 0


def test_prefix_equals_full_prompt_bf16(bf16_case, mid):
    cfg, _ = mid
    m, d, vp, full = bf16_case
    out = _single(m, d, vp=vp)
    assert out.sequences.tolist() == full.sequences.tolist() and out.sequences[0, P_LEN + SUFFIX:].tolist() == d["forced"][0]
    assert _wav(out).shape == _wav(full).shape == (3 * cfg.hop,)
    err = rel_rms(_wav(out), _wav(full), "generate(voice_prefix=) vs full-prompt generate(), mid bf16, waveform")
    print(f"prefix vs full prompt, mid bf16: waveform rel RMS {err:.3e}")
    assert err < 2e-2, f"prefix vs full prompt (bf16): waveform rel RMS {err:.3e}"


def test_prefix_equals_full_prompt_fp32(tiny_cfg, tiny_weights):
    """`tiny` in fp32 (head_dim 16: fp32 cache, no transposed value copy) at the bar of the fp32 loop-trace test, 1e-3"""
    _need_gpu()
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    m = M(tiny_cfg, tiny_weights, device="cuda:0", torch_dtype=torch.float32)
    m.set_ddpm_inference_steps(10)
    d = _inputs(tiny_cfg, seed=23)
    full = _single(m, d)
    vp = _prepare(m, d)
    assert vp.k.dtype == torch.float32 and m.engine.kv.vt is None
    out = _single(m, d, vp=vp)
    assert out.sequences.tolist() == full.sequences.tolist()
    err = rel_rms(_wav(out), _wav(full), "generate(voice_prefix=) vs full-prompt generate(), tiny fp32, waveform")
    print(f"prefix vs full prompt, tiny fp32: waveform rel RMS {err:.3e}")
    assert err < 1e-3, f"prefix vs full prompt (fp32): waveform rel RMS {err:.3e}"
    m.engine.close()


def test_the_work_is_actually_skipped(bf16_case, monkeypatch):
    """no voice encode, and the prefill sees the script rows + the negative prompt's row only"""
    m, d, vp, full = bf16_case

    def no_encode(*a, **k):
        raise AssertionError("the voice encode ran although a prefix was given")
    monkeypatch.setattr(m, "_process_speech_inputs", no_encode)
    rows = []
    fwd = m.engine.llm_forward

    def counting(x, *a, **k):
        rows.append(int(x.shape[0]))
        return fwd(x, *a, **k)
    monkeypatch.setattr(m.engine, "llm_forward", counting)
    out = _single(m, d, vp=vp)
    assert sum(rows) == SUFFIX + 1, f"prefill rows with a prefix: {rows}"
    assert out.sequences.tolist() == full.sequences.tolist()
    monkeypatch.undo()
    rows.clear()
    monkeypatch.setattr(m.engine, "llm_forward", counting)
    _single(m, d)
    assert sum(rows) == P_LEN + SUFFIX + 1, f"prefill rows of the full prompt: {rows}"


def test_the_store_is_read_only(bf16_case):
    m, d, vp, _ = bf16_case
    k0, v0 = vp.k.clone(), vp.v.clone()
    a = _single(m, d, vp=vp)
    b = _single(m, d, vp=vp)
    assert torch.equal(a.speech_outputs[0], b.speech_outputs[0]), "two calls with the same prefix must be bit-identical"
    assert torch.equal(vp.k.view(torch.int16), k0.view(torch.int16)) and torch.equal(vp.v.view(torch.int16), v0.view(torch.int16))


def test_prefix_with_chunked_suffix_prefill(bf16_case):
    """prefill_chunk smaller than the script part: the 25 rows after the prefix run as two chunks (16 + 9) at positions P and P + 16"""
    m, d, vp, full = bf16_case
    out = _single(m, d, vp=vp, prefill_chunk=16)
    assert out.sequences.tolist() == full.sequences.tolist()
    err = rel_rms(_wav(out), _wav(full), "generate(voice_prefix=, prefill_chunk=16) vs full-prompt generate(), mid bf16, waveform")
    assert err < 2e-2, f"prefix + chunked suffix vs full prompt: waveform rel RMS {err:.3e}"


def test_prefix_fp8_kv(bf16_case, mid):
    """kv_cache_dtype='fp8': the store holds the staging cache's bf16 values; the scales come from all P + L slots on both paths"""
    cfg, get = mid
    _, d, _, full16 = bf16_case
    m8 = get("kv8")
    full = _single(m8, d)
    sc_full = m8.engine._kv_scale.clone()
    vp = _prepare(m8, d)
    assert vp.k.dtype == torch.bfloat16 and vp.P == P_LEN
    out = _single(m8, d, vp=vp)
    sc_pre = m8.engine._kv_scale.clone()
    assert out.sequences.tolist() == full.sequences.tolist()
    assert torch.equal(sc_pre, sc_full), "the fp8 scales after the prefill must not depend on the prefix path"
    e_w8 = rel_rms(_wav(_single(get("w8"), d)), _wav(full16), "yardstick: weight_quant='fp8' vs plain bf16 on the voice-prefix test call, waveform")
    err = rel_rms(_wav(out), _wav(full), "generate(voice_prefix=) vs full-prompt generate(), mid bf16 + fp8 KV, waveform")
    print(f"prefix vs full prompt, fp8 KV: waveform rel RMS {err:.3e} (weight-only fp8 yardstick {e_w8:.3e})")
    assert err <= e_w8, f"prefix vs full prompt (fp8 KV): waveform rel RMS {err:.3e} exceeds the weight-only fp8 yardstick {e_w8:.3e}"


@pytest.mark.parametrize("quant", ["fp8", "nf4"])
def test_prefix_with_quantised_weights(mid, quant):
    cfg, get = mid
    m = get("w8" if quant == "fp8" else "nf4")
    d = _inputs(cfg)
    full = _single(m, d)
    out = _single(m, d, vp=_prepare(m, d))
    assert out.sequences.tolist() == full.sequences.tolist()
    err = rel_rms(_wav(out), _wav(full), f"generate(voice_prefix=) vs full-prompt generate(), mid bf16 weight_quant={quant}, waveform")
    assert err < 2e-2, f"prefix vs full prompt (weight_quant={quant}): waveform rel RMS {err:.3e}"


def test_prefix_refresh_negative_off_and_streamer(bf16_case):
    """refresh_negative=False and an AudioStreamer: the prefix path delivers the same chunks as it returns, and matches the full prompt"""
    from vibevoice_rocm_amd.streamer import AudioStreamer
    m, d, vp, _ = bf16_case
    full = _single(m, d, refresh_negative=False)
    st = AudioStreamer(batch_size=1)
    out = _single(m, d, vp=vp, refresh_negative=False, audio_streamer=st)
    got = torch.cat([c.reshape(-1) for c in st.get_stream(0)])
    assert torch.equal(got, out.speech_outputs[0][0].cpu())
    assert out.sequences.tolist() == full.sequences.tolist()
    assert rel_rms(_wav(out), _wav(full), "generate(voice_prefix=, refresh_negative=False) vs full prompt, mid bf16, waveform") < 2e-2


@pytest.fixture(scope="module")
def batch_case(mid, bf16_case):
    """3 dialogues in the same voice with different scripts (25 / 18 / 30 tokens), left padded; the single-dialogue prefix calls as reference"""
    cfg, _ = mid
    m, _, _, _ = bf16_case
    d = _inputs(cfg, seed=41, suffixes=(25, 18, 30))
    vp = _prepare(m, d)
    prompts = [torch.cat([d["pre"], s]) for s in d["suffix"]]
    Lp = max(len(p) for p in prompts)
    ids = torch.stack([torch.cat([torch.zeros(Lp - len(p), dtype=torch.long), p]) for p in prompts])
    am = torch.stack([torch.cat([torch.zeros(Lp - len(p), dtype=torch.long), torch.ones(len(p), dtype=torch.long)]) for p in prompts])
    sm = torch.stack([torch.cat([torch.zeros(Lp - len(p), dtype=torch.bool), d["pre_mask"], torch.zeros(len(p) - P_LEN, dtype=torch.bool)]) for p in prompts])
    kw = dict(input_ids=ids, attention_mask=am, speech_input_mask=sm, tokenizer=d["tok"], cfg_scale=2.0, forced_tokens=d["forced"], noise=d["noise"])
    singles = [_single(m, d, b, vp=vp) for b in range(3)]
    return m, d, vp, kw, singles, Lp


def test_batch_on_the_lanes_and_on_the_row_batch(batch_case):
    m, d, vp, kw, singles, Lp = batch_case
    lanes = m.generate(voice_prefix=vp, row_batch=False, **kw)
    rows = m.generate(voice_prefix=vp, row_batch=True, **kw)
    assert (3, 0) in m._rowbatch, "the second call must have run on the row batch"
    assert rows.sequences.tolist() == lanes.sequences.tolist()
    for b in range(3):
        assert lanes.sequences[b, Lp: Lp + len(d["forced"][b])].tolist() == d["forced"][b]
        assert torch.equal(lanes.speech_outputs[b].reshape(-1), singles[b].speech_outputs[0].reshape(-1)), f"dialogue {b}: the lane must equal the single prefix call"
        err = rel_rms(_wav(rows, b), _wav(lanes, b), f"generate(voice_prefix=) 3 dialogues mid bf16, row-batched vs lanes, waveform of dialogue {b}")
        print(f"dialogue {b}: row batch vs lanes rel RMS {err:.3e}")
        assert err < 1e-2, f"dialogue {b}: row batch vs lanes waveform rel RMS {err:.3e}"


def test_batch_with_a_per_dialogue_list(batch_case):
    """[vp, None, vp]: dialogue 1 takes the full path (its voice is encoded, its whole prompt prefilled) and equals its full single call;
    the voice tensors are given as the processor returns them, one row per dialogue, and only dialogue 1's row is encoded"""
    m, d, vp, kw, singles, Lp = batch_case
    full1 = _single(m, d, 1)
    sn = (d["speech_noise"][0].repeat(3), d["speech_noise"][1].repeat(3, 1, 1))
    out = m.generate(voice_prefix=[vp, None, vp], row_batch=False, speech_tensors=d["wav"].repeat(3, 1), speech_masks=d["sm"].repeat(3, 1), speech_noise=sn, **kw)
    for b, ref in ((0, singles[0]), (1, full1), (2, singles[2])):
        assert torch.equal(out.speech_outputs[b].reshape(-1), ref.speech_outputs[0].reshape(-1)), f"dialogue {b}"
    # any other number of voice rows is refused, not guessed at
    with pytest.raises(ValueError, match="holds 1 voices"):
        m.generate(voice_prefix=[vp, None, vp], row_batch=False, speech_tensors=d["wav"], speech_masks=d["sm"], speech_noise=d["speech_noise"], **kw)


def test_refusals(bf16_case, tiny_cfg, tiny_weights):
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    m, d, vp, _ = bf16_case
    ids = torch.cat([d["pre"], d["suffix"][0]])
    mask = torch.cat([d["pre_mask"], torch.zeros(SUFFIX, dtype=torch.bool)])
    kw = dict(tokenizer=d["tok"], cfg_scale=2.0, forced_tokens=d["forced"][0], noise=d["noise"][0], voice_prefix=vp)
    bad = ids.clone()
    bad[11] += 1
    with pytest.raises(ValueError, match="first at 11"):
        m.generate(input_ids=bad[None], speech_input_mask=mask[None], **kw)
    with pytest.raises(ValueError, match="longer than the prefix"):
        m.generate(input_ids=d["pre"][None], speech_input_mask=d["pre_mask"][None], **kw)
    late = mask.clone()
    late[P_LEN + 2] = True
    with pytest.raises(ValueError, match=f"position {P_LEN + 2}"):
        m.generate(input_ids=ids[None], speech_input_mask=late[None], **kw)
    other = M(tiny_cfg, tiny_weights, device="cuda:0", torch_dtype=torch.float32)
    with pytest.raises(ValueError, match="other shapes"):
        other.generate(input_ids=ids[None] % 100, speech_input_mask=mask[None], **dict(kw, tokenizer=_Tok(tiny_cfg.vocab)))
    other.engine.close()
    # a refused call leaves the model usable
    out = m.generate(input_ids=ids[None], speech_input_mask=mask[None], **kw)
    assert out.sequences[0, P_LEN + SUFFIX:].tolist() == d["forced"][0]
