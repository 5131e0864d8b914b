"""Host side of the voice prefix cache (no GPU): `VibeVoiceProcessor.voice_prefix` against `__call__` under the synthetic tokenizer, `__call__`
itself against the prompt assembly as it stood before the voice-only head was factored out (restated here piece by piece), the checks
generate(voice_prefix=...) makes before it touches the GPU (voice_prefix.check / per_dialogue), and the ABI table entry of vv_kv_copy."""
import ctypes as C

import numpy as np
import pytest
import torch

from vibevoice_rocm_amd import _lib
from vibevoice_rocm_amd import voice_prefix as VP
from vibevoice_rocm_amd.processor import SyntheticTokenizer, VibeVoiceProcessor

SCRIPTS = {
    1: "Speaker 1: One voice reads the whole script.\nSpeaker 1: And a second line.",
    2: "Speaker 1: Hello there.\nSpeaker 2: Hi, how are you?\nSpeaker 1: Fine.",
    4: "Speaker 1: a\nSpeaker 2: bb\nSpeaker 3: ccc\nSpeaker 4: dddd\nSpeaker 2: again",
}


def _voices(n, hop=3200):
    g = np.random.default_rng(7)
    return [(0.1 * g.standard_normal(k * hop - 123)).astype(np.float32) for k in (3, 2, 4, 1)[:n]]


def _processor():
    return VibeVoiceProcessor(tokenizer=SyntheticTokenizer(1024))


def _old_process_single(p, text, voice_samples):
    """ids and mask of one prompt as `_process_single` assembled them before `_prompt_head` existed"""
    tok = p.tokenizer
    parsed = p._parse_script(text)
    speakers = list(set(s for s, _ in parsed))
    full = tok.encode(p.system_prompt)
    mask = [False] * len(full)
    speech = []
    if voice_samples:
        vt, speech, vm = p._create_voice_prompt(voice_samples[: len(speakers)])
        full += vt
        mask += vm
    t = tok.encode(" Text input:\n", add_special_tokens=False)
    full += t
    mask += [False] * len(t)
    for sid, stext in parsed:
        t = tok.encode(f" Speaker {sid}:{stext}\n", add_special_tokens=False)
        full += t
        mask += [False] * len(t)
    t = tok.encode(" Speech output:\n", add_special_tokens=False) + [tok.speech_start_id]
    full += t
    mask += [False] * len(t)
    return full, mask, speech


@pytest.mark.parametrize("n", [1, 2, 4])
def test_voice_prefix_is_an_exact_prefix_of_call(n):
    p = _processor()
    voices = _voices(n)
    full = p(text=SCRIPTS[n], voice_samples=voices, return_tensors="pt")
    pre = p.voice_prefix(voices)
    P = pre["input_ids"].shape[1]
    assert pre["input_ids"].shape == pre["speech_input_mask"].shape == (1, P) and 0 < P < full["input_ids"].shape[1]
    assert torch.equal(pre["input_ids"][0], full["input_ids"][0, :P])
    assert torch.equal(pre["speech_input_mask"][0], full["speech_input_mask"][0, :P])
    assert not bool(full["speech_input_mask"][0, P:].any()), "every voice placeholder lies inside the prefix"
    assert int(pre["speech_input_mask"].sum()) == sum(-(-v.shape[0] // 3200) for v in voices)
    assert torch.equal(pre["speech_tensors"], full["speech_tensors"]) and torch.equal(pre["speech_masks"], full["speech_masks"])
    # the prefix ends with " Text input:\n" and the suffix starts with the first script line
    tail = p.tokenizer.encode(" Text input:\n", add_special_tokens=False)
    assert pre["input_ids"][0, -len(tail):].tolist() == tail


@pytest.mark.parametrize("n", [1, 2, 4])
def test_call_is_unchanged_by_the_refactoring(n):
    p = _processor()
    voices = _voices(n)
    ids, mask, speech = _old_process_single(p, SCRIPTS[n], voices)
    out = p(text=SCRIPTS[n], voice_samples=voices, return_tensors="pt")
    assert out["input_ids"][0].tolist() == ids and out["speech_input_mask"][0].tolist() == mask
    want = p.prepare_speech_inputs(speech, return_tensors="pt")
    assert torch.equal(out["speech_tensors"], want["padded_speeches"]) and torch.equal(out["speech_masks"], want["speech_masks"])
    # a left-padded batch of all three scripts, and a prompt without voices
    texts = [SCRIPTS[k] for k in (1, 2, 4)]
    vs = [_voices(k) for k in (1, 2, 4)]
    batch = p(text=texts, voice_samples=vs, return_tensors="pt")
    olds = [_old_process_single(p, t, v) for t, v in zip(texts, vs)]
    mx = max(len(o[0]) for o in olds)
    for b, (ids, mask, _) in enumerate(olds):
        pad = mx - len(ids)
        assert batch["input_ids"][b].tolist() == [p.tokenizer.pad_id] * pad + ids
        assert batch["speech_input_mask"][b].tolist() == [False] * pad + mask
        assert batch["attention_mask"][b].tolist() == [0] * pad + [1] * len(ids)
    plain = p(text=SCRIPTS[2], return_tensors="pt")
    ids, mask, speech = _old_process_single(p, SCRIPTS[2], None)
    assert plain["input_ids"][0].tolist() == ids and not speech and plain["speech_tensors"] is None


def test_a_script_with_fewer_speakers_has_another_prefix():
    """`__call__` uses one sample per speaker of the script: two samples with a one-speaker script give the one-voice prefix"""
    p = _processor()
    voices = _voices(2)
    full = p(text=SCRIPTS[1], voice_samples=voices, return_tensors="pt")
    one, two = p.voice_prefix(voices[:1]), p.voice_prefix(voices)
    P1, P2 = one["input_ids"].shape[1], two["input_ids"].shape[1]
    assert torch.equal(one["input_ids"][0], full["input_ids"][0, :P1])
    assert not torch.equal(two["input_ids"][0], full["input_ids"][0, :P2])
    with pytest.raises(ValueError):
        p.voice_prefix([])


def _store(P=10, layers=2, kv_heads=2, head_dim=16, dtype=torch.float32):
    shape = VP.store_shape(layers, kv_heads, head_dim, P)
    k, v = torch.zeros(shape, dtype=dtype), torch.zeros(shape, dtype=dtype)
    return VP.VoicePrefix(ids=torch.arange(P), P=P, k=k, v=v, kv=VP.describe(k, v), nbytes=2 * k.numel() * k.element_size())


def test_store_description():
    vp = _store(P=70, dtype=torch.bfloat16)
    assert tuple(vp.k.shape) == (2, 1, 2, 128, 16) and vp.kv.rows == 1 and vp.kv.s_max == 128 and vp.kv.kvdt == _lib.VV_BF16
    assert not vp.kv.vt and not vp.kv.kscale and vp.kv.k == vp.k.data_ptr() and vp.nbytes == 2 * 2 * 2 * 128 * 16 * 2
    assert (vp.layers, vp.kv_heads, vp.head_dim, vp.dtype) == (2, 2, 16, torch.bfloat16)
    assert VP.store_shape(2, 2, 16, 64)[3] == 64 and VP.store_shape(2, 2, 16, 65)[3] == 128 and VP.store_shape(2, 2, 16, 3)[3] == 64


def test_check_names_what_differs():
    vp = _store()
    model = dict(layers=2, kv_heads=2, head_dim=16, dtype=torch.float32)
    ids = torch.arange(15)
    mask = torch.zeros(15, dtype=torch.bool)
    mask[3:6] = True
    VP.check(vp, ids, mask, **model)
    VP.check(vp, ids, None, **model)
    bad = ids.clone()
    bad[4] = 99
    with pytest.raises(ValueError, match="first at 4"):
        VP.check(vp, bad, mask, **model)
    with pytest.raises(ValueError, match="longer than the prefix"):
        VP.check(vp, ids[:10], mask[:10], **model)
    late = mask.clone()
    late[10] = True
    with pytest.raises(ValueError, match="position 10"):
        VP.check(vp, ids, late, **model)
    with pytest.raises(ValueError, match="other shapes"):
        VP.check(vp, ids, mask, **dict(model, kv_heads=4))
    with pytest.raises(ValueError, match="other shapes"):
        VP.check(vp, ids, mask, **dict(model, dtype=torch.bfloat16))


def test_per_dialogue():
    vp = _store()
    assert VP.per_dialogue(None, 3) is None and VP.per_dialogue([None, None], 2) is None
    assert VP.per_dialogue(vp, 3) == [vp, vp, vp]
    assert VP.per_dialogue([vp, None, vp], 3) == [vp, None, vp]
    with pytest.raises(ValueError, match="one entry per dialogue"):
        VP.per_dialogue([vp, None], 3)
    with pytest.raises(ValueError, match="VoicePrefix"):
        VP.per_dialogue(["voice.wav"], 1)


def test_vv_kv_copy_is_in_the_abi_table():
    res, args = _lib.PROTOTYPES["vv_kv_copy"]
    assert res is C.c_int and args == [C.POINTER(_lib.KV), C.c_int, C.POINTER(_lib.KV), C.c_int, C.c_int, C.c_void_p]
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vv_hip.h")).read()
    assert "int vv_kv_copy(const vv_kv* src, int src_row, const vv_kv* dst, int dst_row, int len, vv_stream_t stream);" in hdr
