"""Packed prompt prefill on the GPU: RowBatch.prefill_packed / vv_llm_prefill_packed against the per-dialogue prefill, then generate(),
a single dialogue and a serving session with packed_prefill on against off.

Model: from_synthetic(VVConfig.preset("mid")), bf16 - hidden 512, qkv 1024, inter 1536, head_dim 128 - with vv_tune("gemm_packed_rows", 64)
for the module, so every LLM matrix of a packed pass runs on gemm_packed_kernel and the attention on the matrix cores.  Three dialogues of 33,
64 and 47 prompt rows: the segment ends fall inside 32-query attention tiles, the 144 prompt rows + 3 negative rows cross a 128-row GEMM tile.

The two paths compute the same function; what differs is which GEMM / attention route every row takes, i.e. the summation order of bf16 products.
The project already accepts one such change - the same prompt prefilled in chunks of 16 rows against one chunk - so that comparison, measured in
the same test on the same dialogues, is the yardstick: every packed figure (rel RMS of K and V over slots [0, len) of each cache row, of
hidden[2 b] and hidden[2 b + 1]) stays under 4 x the largest yardstick figure.  4: two GEMM summation orders differ instead of one and the
attention tile boundaries move too; a row at a wrong position or on a wrong cache row costs order 1.  Both figures go to the parity record.
Waveform bars are the ones the project has for "same prompt, another prefill split" (2e-2, tests/test_hip_voice_prefix.py) and for a session
against another serving of the same dialogues (1e-2, tests/test_hip_session.py).

Measured on the MI355X: yardstick 3.96e-3 (hidden[1] of dialogue 0), so the bar is 1.58e-2; the packed path's worst figure is 2.22e-3 (hidden[0] of
dialogue 0) in one pass, in three passes and with the prefix alike; dialogues 0 and 2 bit-identical under a changed dialogue 1; waveforms 4.9e-3 ..
5.8e-3 (3 and 6 dialogues), 5.8e-3 (one dialogue), 5.9e-3 at most (session)."""
import ctypes as C

import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

LENS = (33, 64, 47)
SENTINEL = 77.0            # exact in bf16; no K / V value of these prompts comes near it
VV_E_ARG, VV_E_UNSUPPORTED = -1, -3
P_LEN = 40                 # voice-prefix rows of the prefix case


class _Tok:
    def __init__(self, v):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = v - 4, v - 3, v - 2, v - 1
        self.bos_token_id = None
        self.pad_id = 0


@pytest.fixture(scope="module")
def mid():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    cfg = VVConfig.preset("mid")
    m = M.from_synthetic(cfg, seed=777)
    m.set_ddpm_inference_steps(10)
    lib = L.load()
    L.check(lib.vv_tune(b"gemm_packed_rows", 64), "vv_tune")
    yield cfg, m
    L.check(lib.vv_tune(b"gemm_packed_rows", -1), "vv_tune")
    m.release_lanes()
    m.engine.close()


def _row_batch(m, s_max=128):
    """a fresh 3-dialogue RowBatch on the model's lanes, its K / V filled with the sentinel"""
    from vibevoice_rocm_amd.rowbatch import RowBatch
    V = m.config.vocab
    rb = RowBatch([m._lane(b) for b in range(3)], stream=m.engine.stream)
    rb.begin(s_max, [V - 4, V - 3, V - 2, V - 1], 1.0)
    with torch.cuda.stream(rb.stream):
        rb._kv_t[0].fill_(SENTINEL)
        rb._kv_t[1].fill_(SENTINEL)
    return rb


def _snapshot(rb):
    rb.stream.synchronize()
    return dict(k=rb._kv_t[0].float().cpu(), v=rb._kv_t[1].float().cpu(), hidden=rb.hidden.cpu().clone(), lens=rb.lens.cpu().tolist())


def _figures(got, ref, lens, tag, record=True):
    """{(dialogue, quantity): rel RMS} over the filled slots of both cache rows of every dialogue and its two hidden rows"""
    out = {}
    for b, n in enumerate(lens):
        for row, ln, name in ((2 * b, n, "pos"), (2 * b + 1, 1, "neg")):
            for q in ("k", "v"):
                out[(b, f"{q}_{name}")] = rel_rms(got[q][:, row, :, :ln].numpy(), ref[q][:, row, :, :ln].numpy(),
                                                  f"{tag}: {q.upper()} of cache row {row} (dialogue {b}), slots [0, {ln})" if record else None)
            out[(b, f"hidden_{name}")] = rel_rms(got["hidden"][row].numpy(), ref["hidden"][row].numpy(), f"{tag}: hidden[{row}] (dialogue {b})" if record else None)
    return out


@pytest.fixture(scope="module")
def case(mid):
    """embeddings of the three dialogues, the negative row, the per-dialogue prefill (one chunk) as reference and the chunk-16 yardstick:
    computed once, shared, never modified"""
    cfg, m = mid
    g = torch.Generator().manual_seed(5)
    emb = [(0.5 * torch.randn(n, cfg.hidden, generator=g)).cuda() for n in LENS]
    other = (0.5 * torch.randn(LENS[1], cfg.hidden, generator=g)).cuda()
    neg = m.engine.embed_ids(torch.tensor([cfg.vocab - 4]))
    snaps = {}
    for chunk in (1024, 16):
        rb = _row_batch(m)
        for b in range(3):
            rb.prefill(b, emb[b], chunk=chunk, neg_embed=neg)
        snaps[chunk] = _snapshot(rb)
        rb.close()
    yard = _figures(snaps[16], snaps[1024], LENS, "yardstick: prefill(chunk=16) vs prefill(chunk=1024), mid bf16")
    return dict(emb=emb, other=other, neg=neg, ref=snaps[1024], yard=max(yard.values()), yard_all=yard)


def _hold(fig, case, what):
    bar = 4 * case["yard"]
    worst = max(fig, key=fig.get)
    print(f"{what}: worst figure {fig[worst]:.3e} at {worst}; yardstick (chunk 16 vs 1024) {case['yard']:.3e}; bar {bar:.3e}")
    for key, v in fig.items():
        assert v < bar, f"{what}: {key} rel RMS {v:.3e} >= 4 x yardstick {case['yard']:.3e}"


def _exact(snap, lens, P=(0, 0, 0)):
    """slots past every row's length keep the sentinel, lens are exact (the negative rows' stay 0 until commit_negative)"""
    assert snap["lens"] == [v for b, n in enumerate(lens) for v in (P[b] + n, 0)]
    for b, n in enumerate(lens):
        for row, ln in ((2 * b, P[b] + n), (2 * b + 1, 1)):
            for q in ("k", "v"):
                assert bool((snap[q][:, row, :, ln:] == SENTINEL).all()), f"{q} of cache row {row}: a slot >= {ln} was written"
                assert bool((snap[q][:, row, :, :ln] != SENTINEL).any(-1).all()), f"{q} of cache row {row}: a slot < {ln} was not written"


def test_packed_equals_per_dialogue_prefill(mid, case):
    cfg, m = mid
    rb = _row_batch(m)
    rb.prefill_packed([(b, case["emb"][b], None) for b in (2, 0, 1)], chunk_rows=4096, neg_embed=case["neg"])      # any order in: packed in ascending b
    got = _snapshot(rb)
    assert rb.prefill_passes == 1
    rb.close()
    _exact(got, LENS)
    assert case["yard"] > 0
    _hold(_figures(got, case["ref"], LENS, "prefill_packed (one pass of 147 rows) vs prefill per dialogue, mid bf16"), case, "one pass")


def test_no_cross_talk_between_dialogues(mid, case):
    """dialogue 1's embeddings replaced by others of the same length: dialogues 0 and 2 are bit-identical in K, V and hidden"""
    cfg, m = mid
    snaps = []
    for e1 in (case["emb"][1], case["other"]):
        rb = _row_batch(m)
        rb.prefill_packed([(0, case["emb"][0], None), (1, e1, None), (2, case["emb"][2], None)], neg_embed=case["neg"])
        snaps.append(_snapshot(rb))
        rb.close()
    a, b = snaps
    for row in (0, 1, 4, 5):
        assert torch.equal(a["k"][:, row], b["k"][:, row]) and torch.equal(a["v"][:, row], b["v"][:, row]), f"cache row {row} changed with dialogue 1"
        assert torch.equal(a["hidden"][row], b["hidden"][row]), f"hidden[{row}] changed with dialogue 1"
    assert not torch.equal(a["k"][:, 2], b["k"][:, 2]) and not torch.equal(a["hidden"][2], b["hidden"][2])      # ... and dialogue 1 did change


def test_cuts_inside_a_dialogue(mid, case):
    """chunk_rows=64: three passes (64, 64, 16 + the negatives); dialogue 1's segment is cut at its row 31 and again at its row 95 - 33"""
    cfg, m = mid
    rb = _row_batch(m)
    rb.prefill_packed([(b, case["emb"][b], None) for b in range(3)], chunk_rows=64, neg_embed=case["neg"])
    got = _snapshot(rb)
    assert rb.prefill_passes == 3
    rb.close()
    _exact(got, LENS)
    _hold(_figures(got, case["ref"], LENS, "prefill_packed (chunk_rows=64, three passes) vs prefill per dialogue, mid bf16"), case, "three passes")


def test_a_dialogue_with_a_voice_prefix(mid, case):
    """dialogue 1 restores a 40-slot prefix and prefills only its suffix rows at positions 40 ..: against prefill(prefix=) on it"""
    cfg, m = mid
    eng = m.engine
    V = cfg.vocab
    pre = (0.5 * torch.randn(P_LEN, cfg.hidden, generator=torch.Generator().manual_seed(9))).cuda()
    eng.begin_sequence(128, [V - 4, V - 3, V - 2, V - 1])
    eng.prefill(pre)
    vp = eng.save_prefix(torch.arange(P_LEN))
    items = [(0, case["emb"][0], None), (1, case["emb"][1], vp), (2, case["emb"][2], None)]
    ref_rb = _row_batch(m, 192)
    for b, e, p in items:
        ref_rb.prefill(b, e, neg_embed=case["neg"], prefix=p)
    ref = _snapshot(ref_rb)
    ref_rb.close()
    rb = _row_batch(m, 192)
    rb.prefill_packed(items, neg_embed=case["neg"])
    got = _snapshot(rb)
    assert rb.prefill_passes == 1
    rb.close()
    _exact(got, LENS, P=(0, P_LEN, 0))
    assert torch.equal(got["k"][:, 2, :, :P_LEN], ref["k"][:, 2, :, :P_LEN])                         # the restored slots are copies
    _hold(_figures(got, ref, (LENS[0], P_LEN + LENS[1], LENS[2]), "prefill_packed with a voice prefix on dialogue 1 vs prefill(prefix=), mid bf16"), case, "prefix")


# ---- generate(), one dialogue, a session ---------------------------------------------------------------------------------------------------
def _batch(cfg, B, seed=23):
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(seed)
    lens = [LENS[b % 3] + 2 * (b // 3) for b in range(B)]
    prompts = [torch.cat([torch.randint(1, cfg.vocab - 8, (n - 1,), generator=g), torch.tensor([S])]) for n in lens]
    Lp = max(lens)
    ids = torch.stack([torch.cat([torch.zeros(Lp - len(p), dtype=torch.long), p]) for p in prompts])
    am = torch.stack([torch.cat([torch.zeros(Lp - len(p), dtype=torch.long), torch.ones(len(p), dtype=torch.long)]) for p in prompts])
    forced = [[[D, D, D, E, EOS], [D, D, E, EOS], [D, E, S, D, D, E, EOS]][b % 3] for b in range(B)]
    noise = torch.randn(B, 4, cfg.latent, generator=g)
    return tok, prompts, dict(input_ids=ids, attention_mask=am, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise), forced


def _passes(m):
    return sum(rb.prefill_passes for rb in m._rowbatch.values())


def _wav(out, b=0):
    return out.speech_outputs[b].reshape(-1).float().cpu().numpy()


@pytest.mark.parametrize("B, passes", [(3, 1), (6, 2)])
def test_generate_packed_vs_per_dialogue(mid, B, passes):
    """3 dialogues (one row batch) and 6 (two row batches at width 4): forced schedules, injected noise; packed_prefill=True makes one pass
    per row batch and the waveforms agree with the per-dialogue prefill to the bar of another prefill split"""
    cfg, m = mid
    tok, prompts, kw, forced = _batch(cfg, B)
    want = m.generate(**kw)
    n0 = _passes(m)
    got = m.generate(packed_prefill=True, **kw)
    assert _passes(m) - n0 == passes
    assert got.sequences.tolist() == want.sequences.tolist()
    for b in range(B):
        err = rel_rms(_wav(got, b), _wav(want, b), f"generate(packed_prefill=True) vs False, {B} dialogues mid bf16, waveform of dialogue {b}")
        print(f"B={B} dialogue {b}: waveform rel RMS {err:.3e}")
        assert err < 2e-2, f"B={B}, dialogue {b}: waveform rel RMS {err:.3e}"
    m.generate(**kw)
    assert _passes(m) - n0 == passes                                   # off by default: the next call packs nothing


def test_one_dialogue_takes_the_same_entry(mid):
    cfg, m = mid
    tok, prompts, kw, forced = _batch(cfg, 3)
    one = dict(input_ids=prompts[1][None], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[1], noise=kw["noise"][1])
    want = m.generate(**one)
    n0 = m.engine.prefill_passes
    got = m.generate(packed_prefill=True, **one)
    assert m.engine.prefill_passes - n0 == 1 and got.sequences.tolist() == want.sequences.tolist()
    err = rel_rms(_wav(got), _wav(want), "generate(packed_prefill=True) vs False, one dialogue of 64 prompt rows, mid bf16, waveform")
    assert err < 2e-2, f"waveform rel RMS {err:.3e}"
    with pytest.raises(ValueError, match="packed_prefill_rows"):
        m.generate(packed_prefill=True, packed_prefill_rows=8, **one)


def test_session_admits_queued_requests_in_one_pass(mid):
    """three requests submitted before the first step of a 4-slot session: one packed pass; a request submitted mid-flight is admitted alone;
    every waveform against the session without the flag"""
    cfg, m = mid
    tok, prompts, kw, forced = _batch(cfg, 4, seed=29)
    outs = {}
    for packed in (False, True):
        with m.open_session(tokenizer=tok, slots=4, max_context=256, device_noise=False, packed_prefill=packed) as sess:
            rb = sess.driver.groups[0][0]
            n0 = rb.prefill_passes
            hs = [sess.submit(input_ids=prompts[i][None], cfg_scale=2.0, forced_tokens=forced[i], noise=kw["noise"][i]) for i in range(3)]
            assert sess.step() and [h.slot for h in hs] == [0, 1, 2]
            assert rb.prefill_passes - n0 == (1 if packed else 0)
            hs.append(sess.submit(input_ids=prompts[3][None], cfg_scale=2.0, forced_tokens=forced[3], noise=kw["noise"][3]))
            assert sess.step() and hs[3].slot == 3
            assert rb.prefill_passes - n0 == (2 if packed else 0)
            assert len(sess.admission_ms) == (2 if packed else 4)
            sess.run()
            outs[packed] = [h.result() for h in hs]
    for i in range(4):
        assert outs[True][i].sequences.tolist() == outs[False][i].sequences.tolist()
        err = rel_rms(_wav(outs[True][i]), _wav(outs[False][i]), f"session packed_prefill=True vs False, mid bf16, waveform of dialogue {i}")
        print(f"session dialogue {i}: waveform rel RMS {err:.3e}")
        assert err < 1e-2, f"session dialogue {i}: waveform rel RMS {err:.3e}"


def test_constructor_keyword_and_default(mid):
    from vibevoice_rocm_amd.modeling import PACKED_PREFILL_ROWS
    cfg, m = mid
    assert m.packed_prefill is False and m.packed_prefill_rows == PACKED_PREFILL_ROWS


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_version_and_refusals(mid):
    """the two symbols exist, the ABI version did not move, and bad arguments return the documented codes without a launch"""
    from vibevoice_rocm_amd import _lib as L
    cfg, m = mid
    lib, eng = L.load(), m.engine
    assert lib.vv_abi_version() == 6
    assert hasattr(lib, "vv_llm_prefill_packed") and hasattr(lib, "vv_llm_prefill_packed_ws_bytes")
    llm = C.byref(eng.w.llm)
    assert lib.vv_llm_prefill_packed_ws_bytes(llm, 147) == lib.vv_llm_ws_bytes(llm, 147) > 0
    V = cfg.vocab
    eng.begin_sequence(128, [V - 4, V - 3, V - 2, V - 1])
    R, H = 70, cfg.hidden
    with torch.cuda.stream(eng.stream):
        x = torch.randn(R, H, device="cuda")
        lens = torch.arange(R, dtype=torch.int32, device="cuda")
        rows = torch.zeros(R, dtype=torch.int32, device="cuda")
        sel = torch.tensor([R - 1], dtype=torch.int32, device="cuda")
        out = torch.full((1, H), float("nan"), device="cuda")
        ws = torch.empty(lib.vv_llm_prefill_packed_ws_bytes(llm, R), dtype=torch.uint8, device="cuda")
    kv = C.byref(eng.kv)

    def call(m_=llm, kv_=kv, x_=x.data_ptr(), lens_=lens.data_ptr(), rows_=rows.data_ptr(), sel_=sel.data_ptr(), nsel=1, out_=out.data_ptr(), ws_=ws.data_ptr()):
        return lib.vv_llm_prefill_packed(m_, kv_, x_, H, R, lens_, rows_, sel_, nsel, out_, H, ws_, eng.sp)

    for bad in (dict(m_=None), dict(kv_=None), dict(x_=None), dict(lens_=None), dict(rows_=None), dict(sel_=None), dict(out_=None), dict(ws_=None), dict(nsel=0),
                dict(nsel=-2)):
        assert call(**bad) == VV_E_ARG, bad
        assert "vv_llm_prefill_packed" in lib.vv_last_error().decode()
    kv8 = L.KV.from_buffer_copy(eng.kv)
    kv8.kvdt = L.VV_FP8
    assert call(kv_=C.byref(kv8)) == VV_E_UNSUPPORTED and "fp8" in lib.vv_last_error().decode()
    eng.stream.synchronize()
    assert bool(torch.isnan(out).all())
    assert call() == 0
    eng.stream.synchronize()
    assert bool(torch.isfinite(out).all())
