"""mxfp6_lean=True at the `mid` preset (bf16): the LLM's matrices exist as MXFP6 codes alone and every prompt pass of 3 or more rows runs the
GEMM on the codes (csrc/vv_gemm_mx6.hip) - against the same model with its bf16 copies, which computes with exactly the same effective weights
through the bf16 GEMM routes.  The MXFP6 image of tests/test_hip_mxfp4_lean.py.

Bars: 2e-2 waveform rel RMS where the same values go through another GEMM route (the bar of the voice-prefix and packed-prefill comparisons),
1e-2 for the row batch against the lanes and for a session against generate() alone (the literals tests/test_hip_rowbatch_mxfp6.py asserts
for those two comparisons; it has no named constant to import).  Forced tokens, 8 frames, one seed throughout.

Every model of this module is built after the engines earlier modules left behind have handed their HIP streams back, and is torn down when
the module ends (the `mid` fixture of tests/test_hip_rowbatch_mxfp6.py says why).
"""
import ctypes as C
import gc

import pytest
import torch

from conftest import rel_rms
from test_hip_rowbatch_mxfp6 import _Tok, _idle_streams_back, _mid_model, _padded

ROUTE_BAR = 2e-2
ROWS_VS_LANES_BAR = 1e-2       # test_generate_mxfp6_row_batch_vs_lanes_and_oracle, test_session_mxfp6_vs_generate_alone
VV_E_UNSUPPORTED = -3
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _stream_pool_as_found():
    """This module builds three models and their lanes - up to six engines at once - from the recycle pool of HIP streams (engine.py,
    _IDLE_STREAMS), a stack.  When it ends, every one of them is back in the pool, but in another order; the modules that follow pop their
    lanes' streams from the top of that stack, and torch hands its 32 streams out round-robin, so two entries of a long-lived pool can be the
    same stream: which entries end up side by side is not this module's to change.  The pool is therefore put back exactly as it was found,
    provided nothing of it is still in use (set up before the models' fixtures, torn down after them)."""
    if not torch.cuda.is_available():
        yield
        return
    from vibevoice_rocm_amd import engine
    _idle_streams_back()
    pool = engine._IDLE_STREAMS.setdefault("cuda:0", [])
    found = list(pool)
    yield
    gc.collect()
    torch.cuda.empty_cache()
    back = {s.cuda_stream for s in pool}
    drawn = len(pool) - len(found)
    print(f"stream pool: {len(found)} found, {len(pool)} at the end ({drawn} drawn from torch by this module)")
    if all(s.cuda_stream in back for s in found):      # streams this module had to draw go to the bottom: the top of the stack is as it was
        pool[:] = [s for s in pool if s.cuda_stream not in {f.cuda_stream for f in found}] + found


def _model_fixture(**kw):
    @pytest.fixture(scope="module")
    def fx():
        if not torch.cuda.is_available():
            pytest.skip("needs a GPU")
        _idle_streams_back()
        box = list(_mid_model(**kw))      # [cfg, model]: a list, so that the fixture's cached value does not keep the model alive below
        yield box
        box.pop().release_lanes()
        gc.collect()
        torch.cuda.empty_cache()
    return fx


plain = _model_fixture()
lean = _model_fixture(mxfp6_lean=True)
lean_rb = _model_fixture(mxfp6_lean=True, mxfp6_row_batch=True)


def _one(cfg, n_prompt, seed):
    tok = _Tok(cfg.vocab)
    D, E, EOS, S = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id, tok.speech_start_id
    g = torch.Generator().manual_seed(seed)
    ids = torch.cat([torch.randint(0, 1000, (n_prompt - 1,), generator=g), torch.tensor([S])])[None]
    return dict(input_ids=ids, tokenizer=tok, cfg_scale=2.0, forced_tokens=[D] * 8 + [E, EOS], noise=torch.randn(8, cfg.latent, generator=g))


def _wave_err(a, r, what):
    assert a.shape == r.shape
    err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what=what)
    print(f"{what}: {err:.3e}")
    return err


@pytest.mark.parametrize("n_prompt", [80, 20])
def test_one_dialogue_lean_vs_bf16_copies(plain, lean, n_prompt):
    """80 prompt rows: the prefill (R >= 64), which reads the bf16 copies on the model that has them; 20 rows: the short pass that model runs
    on its few-row bf16 routes.  The lean model runs both on the GEMM on the codes."""
    cfg, mp = plain
    _, ml = lean
    kw = _one(cfg, n_prompt, 7)
    want, got = mp.generate(**kw), ml.generate(**kw)
    assert got.sequences.tolist() == want.sequences.tolist()
    err = _wave_err(got.speech_outputs[0], want.speech_outputs[0], f"mid mxfp6, {n_prompt}-row prompt: lean vs bf16 copies, waveform")
    assert err <= ROUTE_BAR, f"waveform rel RMS {err:.3e}"


def _three(cfg, seed=64):
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(seed)
    ids, mask, _ = _padded(tok, [40, 31, 36], g)
    forced = [[D] * 5 + [E, EOS], [D] * 3 + [E, S, D, D, E, EOS], [D] * 2 + [E, EOS]]
    noise = torch.randn(3, 8, cfg.latent, generator=g)
    return tok, ids, mask, forced, noise


def test_two_dialogues_on_lean_lanes_equal_the_singles_bit_for_bit(lean):
    """without mxfp6_row_batch a batch runs on the lanes, as a model with bf16 copies does: each dialogue is then the single-dialogue engine on
    its own prompt, and a prompt row's GEMM result does not depend on what else is in flight"""
    cfg, m = lean
    tok, ids, mask, forced, noise = _three(cfg)
    m.release_lanes()
    both = m.generate(input_ids=ids[:2], attention_mask=mask[:2], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[:2], noise=noise[:2])
    assert not m._rowbatch, "a lean model without mxfp6_row_batch took the row-batched path"
    for b in range(2):
        n = int(mask[b].sum())
        one = m.generate(input_ids=ids[b: b + 1, -n:], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[b], noise=noise[b])
        assert torch.equal(both.speech_outputs[b], one.speech_outputs[0]), f"dialogue {b}: the lane and the single run differ"
    with pytest.raises(ValueError, match="weight_quant='mxfp6'"):
        m.open_session(tokenizer=tok, max_context=256)
    m.release_lanes()


def test_lean_row_batch_vs_lean_lanes(lean_rb):
    cfg, m = lean_rb
    tok, ids, mask, forced, noise = _three(cfg)
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    m.release_lanes()
    lanes = m.generate(row_batch=False, **kw)
    assert not m._rowbatch
    rows = m.generate(**kw)
    assert (3, 0) in m._rowbatch, "mxfp6_row_batch=True on 3 dialogues did not take the row-batched path"
    assert rows.sequences.tolist() == lanes.sequences.tolist()
    for b in range(3):
        err = _wave_err(rows.speech_outputs[b], lanes.speech_outputs[b], f"mid mxfp6 lean, 3 dialogues row-batched vs lanes, dialogue {b}")
        assert err < ROWS_VS_LANES_BAR, f"dialogue {b}: waveform rel RMS {err:.3e}"
    packed = m.generate(packed_prefill=True, **kw)
    assert packed.sequences.tolist() == rows.sequences.tolist()
    for b in range(3):
        err = _wave_err(packed.speech_outputs[b], rows.speech_outputs[b], f"mid mxfp6 lean, packed prefill vs per-dialogue prefill, dialogue {b}")
        assert err <= ROUTE_BAR, f"dialogue {b}: waveform rel RMS {err:.3e}"
    m.release_lanes()


def test_lean_session_vs_generate_alone(lean_rb):
    cfg, m = lean_rb
    kw = _one(cfg, 44, 61)
    tok = kw.pop("tokenizer")
    m.release_lanes()
    with m.open_session(tokenizer=tok, slots=2, max_context=256, device_noise=False) as sess:
        h = sess.submit(input_ids=kw["input_ids"], cfg_scale=kw["cfg_scale"], forced_tokens=kw["forced_tokens"], noise=kw["noise"])
        sess.run()
    assert h.done
    want = m.generate(tokenizer=tok, **kw)
    got = h.result()
    assert got.sequences.tolist() == want.sequences.tolist()
    err = _wave_err(got.speech_outputs[0], want.speech_outputs[0], "mid mxfp6 lean, one request through a session vs generate() alone")
    assert err < ROWS_VS_LANES_BAR, f"waveform rel RMS {err:.3e}"
    m.release_lanes()


def _llm_names(cfg):
    names = []
    for l in range(cfg.layers):
        q = f"model.language_model.layers.{l}."
        names += [q + "self_attn.qkv_proj.weight", q + "self_attn.o_proj.weight"] + [q + f"mlp.{n}_proj.weight" for n in ("gate", "up", "down")]
    return names


def test_memory_is_smaller_by_exactly_the_dropped_copies(plain, lean, lean_rb):
    cfg, mp = plain
    wl = lean[1].engine.w
    rep = wl.lean_report()
    assert rep and all(d["bytes"] == 2 * d["n"] * d["k"] and d["n"] % 16 == 0 and d["k"] % 128 == 0 for d in rep)
    assert {d["name"] for d in rep} == set(_llm_names(cfg)), "the LLM's matrices of mid, and no other, are held as codes alone"
    assert wl.nbytes() == mp.engine.w.nbytes() - sum(d["bytes"] for d in rep)
    print(f"mid mxfp6: nbytes with copies {mp.engine.w.nbytes()}, lean {wl.nbytes()}, lean + row batch {lean_rb[1].engine.w.nbytes()}")
    assert mp.engine.w.lean_report() == []
    for w in (wl, lean_rb[1].engine.w):
        for l in range(cfg.layers):
            lay = w.llm.layer[l]
            assert not (lay.wqkv or lay.wo or lay.wgate or lay.wup or lay.wdown), f"layer {l}: a bf16 pointer is set"
            assert all(q.q and q.scale for q in (lay.q_qkv, lay.q_o, lay.q_gate, lay.q_up, lay.q_down))
    lay = mp.engine.w.llm.layer[0]
    assert lay.wqkv and lay.wo and lay.wgate and lay.wup and lay.wdown


def test_decode_pass_of_4_rows_without_fragment_copies_is_refused_before_any_launch(lean):
    """vv_llm_forward with R = 4 in decode form (cache_rows == NULL) on a lean model without VV_MXFP6_FRAG copies: no resident matrix can serve
    it.  VV_E_UNSUPPORTED naming the lean mode and the keyword that would build the copies; the output, the workspace and the cache are as they
    were"""
    from vibevoice_rocm_amd import _lib as L
    cfg, m = lean
    eng, lib = m.engine, L.load()
    dev, R, S = eng.device, 4, 64
    torch.cuda.synchronize()
    kt = torch.zeros(cfg.layers, R, cfg.kv_heads, S, cfg.head_dim, dtype=torch.bfloat16, device=dev)
    vt = torch.zeros_like(kt)
    kv = L.KV()
    kv.k, kv.v, kv.kvdt, kv.layers, kv.rows, kv.kv_heads, kv.s_max, kv.head_dim = kt.data_ptr(), vt.data_ptr(), L.VV_BF16, cfg.layers, R, cfg.kv_heads, S, cfg.head_dim
    x = torch.randn(R, cfg.hidden, device=dev)
    lens = torch.zeros(R, dtype=torch.int32, device=dev)
    out = torch.full((R, cfg.hidden), float("nan"), device=dev)
    n = lib.vv_llm_ws_bytes(C.byref(eng.w.llm), R)
    assert n > 0
    ws = torch.full((n // 4 + 1,), float("nan"), device=dev)
    torch.cuda.synchronize()
    rc = lib.vv_llm_forward(C.byref(eng.w.llm), C.byref(kv), x.data_ptr(), cfg.hidden, R, lens.data_ptr(), None, out.data_ptr(), cfg.hidden, ws.data_ptr(), None)
    err = lib.vv_last_error().decode()
    assert rc == VV_E_UNSUPPORTED, (rc, err)
    assert "lean" in err and "mxfp6_row_batch" in err, err
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all() and not kt.any() and not vt.any()
    del kt, vt, ws
    gc.collect()
