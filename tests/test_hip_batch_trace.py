"""Batched generate() against the reference's own BATCHED loop (tests/golden/loop_trace_batch_*.npz, oracle/gen/make_golden.py
gen_loop_trace_batch), and the per-dialogue decode tail (vv_llm_tail_batch, vv_llm_tail, vv_advance_lens, vv_argmax_ids) against an fp64
restatement.

The fixture's entries: a - interleaved segments, an early EOS, a speech_start while another sample diffuses (per-sample semantics hold);
b - the guard disagreement of modeling_vibevoice_inference.py:595 / :607 (a non-diffusing sample's negative row replaces its last visible
one); c - the streaming tokenizer cache's all-or-nothing get() (a first-time diffuser restarts the conv states of the whole subset).
generate() reproduces b and c through modeling._BatchCoupling."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_rms

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class _Tok:
    def __init__(self, st, se, sd, eos):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = st, se, sd, eos
        self.bos_token_id = None
        self.pad_id = 0


ENTRIES = ("a", "b", "c")


def _batch_call(m, g, entry, **kw):
    ST, E, D, EOS = [int(v) for v in g["special"]]
    B = g[f"{entry}_ids"].shape[0]
    forced = [g[f"{entry}_s{b}_forced"].tolist() for b in range(B)]
    F = max(g[f"{entry}_s{b}_noise"].shape[0] for b in range(B))
    noise = torch.zeros(B, F, g[f"{entry}_s0_noise"].shape[1])
    for b in range(B):
        n = torch.from_numpy(g[f"{entry}_s{b}_noise"])
        noise[b, : n.shape[0]] = n
    T = lambda k: torch.from_numpy(g[f"{entry}_{k}"])        # noqa: E731
    m.set_ddpm_inference_steps(int(g["n_steps"]))
    out = m.generate(input_ids=T("ids"), attention_mask=T("attention_mask"), speech_tensors=T("voice"), speech_masks=T("speech_masks"),
                     speech_input_mask=T("speech_input_mask"), tokenizer=_Tok(ST, E, D, EOS), cfg_scale=float(g["cfg_scale"]),
                     forced_tokens=forced, noise=noise, speech_noise=(T("std_noise"), T("eps_noise")),
                     generation_config={"do_sample": False}, show_progress_bar=False, **kw)
    return B, out


def _check(g, entry, out, B, bar, what):
    Lp = g[f"{entry}_ids"].shape[1]
    errs = []
    for b in range(B):
        tokens = g[f"{entry}_s{b}_tokens"].tolist()
        assert out.sequences[b, Lp: Lp + len(tokens)].tolist() == tokens, (entry, b)
        want = g[f"{entry}_s{b}_wav"].reshape(-1)
        wav = out.speech_outputs[b][0].float().cpu().numpy()
        assert wav.shape == want.shape, (entry, b, wav.shape, want.shape)
        e = rel_rms(wav, want, what=f"{what}, entry {entry}, sample {b}")
        errs.append(e)
    for b, e in enumerate(errs):
        assert e < bar, f"{what}, entry {entry}, sample {b}: waveform rel RMS {e:.3e} (bar {bar:.0e}); all: {['%.2e' % x for x in errs]}"


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("entry", ENTRIES)
def test_lanes_fp32_vs_reference_batch_trace(tiny_cfg, tiny_weights, graphs, entry):
    """The lanes (row_batch=False), fp32 tiny weights: sequences exact, every waveform within 1e-3 relative RMS of the reference's batched
    loop - the bar of test_generate_loop_vs_reference_trace."""
    _need_gpu()
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    g = load_golden("loop_trace_batch_tiny")
    m = VibeVoiceForConditionalGenerationInference(tiny_cfg, tiny_weights, device="cuda:0", torch_dtype=torch.float32, use_graphs=graphs)
    try:
        B, out = _batch_call(m, g, entry, row_batch=False)
    finally:
        _drop(m)
    _check(g, entry, out, B, 1e-3, f"generate() lanes fp32 tiny, graphs={graphs}, vs reference batched loop")


def test_lanes_do_sample_streams_every_chunk_as_it_returns_it(tiny_cfg, tiny_weights):
    """do_sample on the lanes with an AudioStreamer: every step delivers the previous step's chunks, so 12 frames - more than the 8 slots of
    a lane's host ring - reach the streamer as the samples generate() returns, bit for bit.  (Forced tokens: the non-sampling kernels
    under the sample_fn branch of the loop.)"""
    _need_gpu()
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.streamer import AudioStreamer
    g = load_golden("loop_trace_batch_tiny")
    ST, E, D, EOS = [int(v) for v in g["special"]]
    m = VibeVoiceForConditionalGenerationInference(tiny_cfg, tiny_weights, device="cuda:0", torch_dtype=torch.float32, use_graphs=True)
    st = AudioStreamer(batch_size=2, timeout=5)
    try:
        m.set_ddpm_inference_steps(int(g["n_steps"]))
        out = m.generate(input_ids=torch.from_numpy(g["a_ids"])[:2], attention_mask=torch.from_numpy(g["a_attention_mask"])[:2],
                         tokenizer=_Tok(ST, E, D, EOS), cfg_scale=float(g["cfg_scale"]), forced_tokens=[D] * 12 + [E, EOS],
                         noise=torch.randn(2, 12, tiny_cfg.latent, generator=torch.Generator().manual_seed(3)),
                         generation_config={"do_sample": True}, audio_streamer=st, row_batch=False)
    finally:
        _drop(m)
    assert out.sequences[:, -14:].tolist() == [[D] * 12 + [E, EOS]] * 2
    for b in range(2):
        got = list(st.get_stream(b))
        assert len(got) == 12, (b, len(got))
        assert torch.equal(torch.cat([c.reshape(-1) for c in got]), out.speech_outputs[b][0].float().cpu()), b


def _drop(m):
    """release a model's engines NOW: an Engine collected later by the garbage collector synchronises its stream in __del__, which
    invalidates a graph capture another test may have running on another stream at that moment"""
    torch.cuda.synchronize()
    m.release_lanes()
    del m
    gc.collect()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def mid_bf16():
    _need_gpu()
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("mid")
    # the fixture's reference ran on the synthetic weights rounded to bf16 (vectors too, as a bf16 checkpoint stores them)
    sd = {k: (torch.from_numpy(v).to(torch.bfloat16).float() if v.ndim >= 1 else torch.from_numpy(v)) for k, v in synth_state_dict(cfg, 1234).items()}
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    yield m
    _drop(m)


@pytest.mark.parametrize("entry", ENTRIES)
def test_row_batch_bf16_vs_reference_batch_trace(mid_bf16, entry):
    """The row-batched path, bf16 `mid` weights (the row-batched path serves bf16 only and its matrix-core GEMVs do not take tiny's
    hidden 64, which is why the fixture has a `mid` twin): sequences exact, waveforms within 2e-2 - the bar of
    test_generate_row_batch_mid_bf16_vs_oracle - with the lanes' error recorded next to it."""
    m = mid_bf16
    g = load_golden("loop_trace_batch_mid")
    m.release_lanes()
    B, out = _batch_call(m, g, entry, row_batch=True)
    assert (B, 0) in m._rowbatch, "the row-batched path was not taken"
    _, lanes = _batch_call(m, g, entry, row_batch=False)
    for b in range(B):
        rel_rms(lanes.speech_outputs[b][0].float().cpu().numpy(), g[f"{entry}_s{b}_wav"].reshape(-1),
                what=f"generate() lanes bf16 mid vs reference batched loop, entry {entry}, sample {b}")
    _check(g, entry, lanes, B, 2e-2, "generate() lanes bf16 mid vs reference batched loop")
    _check(g, entry, out, B, 2e-2, "generate() ROW-BATCHED bf16 mid vs reference batched loop")


# ---------------------------------------------------------------------------------------------------------------
# the decode tail
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    from vibevoice_rocm_amd import _lib
    return _lib.load()


def _llm(hidden, wdt, norm_w, eps=1e-6):
    from vibevoice_rocm_amd import _lib as L
    m = L.Llm()
    m.wdt, m.hidden, m.rms_eps, m.final_norm = wdt, hidden, eps, norm_w.data_ptr()
    return m


def _ref_tail(h, norm_w, w, ids, forced, lens, frame, active, tok_start, tok_diff, eps=1e-6):
    """fp64: final RMSNorm of both rows -> logits of row 0 -> first maximum in ascending id order -> forced override -> bookkeeping"""
    h = h.astype(np.float64)
    out = h / np.sqrt(np.mean(h * h, axis=1, keepdims=True) + eps) * norm_w.astype(np.float64)
    lg = w.astype(np.float64) @ out[0]
    _ref_tail.scale = np.abs(w.astype(np.float64)) @ np.abs(out[0])        # sum |w_i,k out_k|: what an fp32 dot product's rounding scales with
    best = min(range(len(ids)), key=lambda i: (-lg[i], ids[i]))
    t = forced if forced >= 0 else int(ids[best])
    lens, frame = list(lens), frame
    if active:
        lens[0] += 1
        if tok_start < 0:
            lens[1] += 1
            frame += t == tok_diff
        elif t == tok_start:
            lens[1] = 0
        elif t == tok_diff:
            lens[1] += 1
            frame += 1
    return out, lg, t, lens, frame


def _w_valid(nv, hidden, bf16, gen):
    w = torch.randn(nv, hidden, generator=gen) / np.sqrt(hidden)
    if bf16:
        w = w.to(torch.bfloat16)
    return w, w.float().numpy()


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("hidden", [64, 512, 1536, 3584, 4096])
def test_llm_tail_batch_vs_fp64(lib, hidden, bf16):
    """vv_llm_tail_batch for B = 1..4 dialogues and nv = 1, 2, 5, 8 ids (not in ascending order): both rows normalised, row 0's logits,
    first maximum / forced token (-1 and real ids mixed), and the bookkeeping of every branch (token == tok_start, == tok_diffusion,
    neither, tok_start < 0); an inactive dialogue keeps lens and frame counter but still gets its rows, logits and token."""
    from vibevoice_rocm_amd import _lib as L
    gen = torch.Generator().manual_seed(hidden + bf16)
    rng = np.random.default_rng(hidden * 2 + bf16)
    norm_w = (1 + 0.1 * torch.randn(hidden, generator=gen)).cuda()
    m = _llm(hidden, L.VV_BF16 if bf16 else L.VV_F32, norm_w)
    worst_row, worst_lg, n_checked = 0.0, 0.0, 0
    for B in range(1, 5):
        for nv in (1, 2, 5, 8):
            w, wn = _w_valid(nv, hidden, bf16, gen)
            ids = rng.permutation(np.arange(100, 100 + 3 * nv, 3))[:nv].astype(np.int32)       # not in ascending order
            for ts_mode in ("start", "diff", "other", "neg"):
                h = torch.randn(2 * B, hidden, generator=gen) * 3
                forced = np.array([-1 if rng.random() < 0.5 else int(rng.choice(ids)) for _ in range(B)], np.int32)
                active = np.array([1 if (b == 0 or rng.random() < 0.6) else 0 for b in range(B)], np.int32)
                lens = rng.integers(0, 50, 2 * B).astype(np.int32)
                frame = rng.integers(0, 9, B).astype(np.int32)
                # the token is tok_start / tok_diffusion / another id in turn, so every bookkeeping branch is taken
                tok_start = int(ids[0]) if ts_mode == "start" else (-1 if ts_mode == "neg" else 7)
                tok_diff = int(ids[0]) if ts_mode in ("diff", "neg") else 8
                if ts_mode in ("start", "diff"):
                    forced[0] = ids[0]
                hd, wd = h.cuda(), w.cuda()
                idd = torch.from_numpy(ids).cuda()
                out = torch.full((2 * B, hidden), float("nan"), device="cuda")
                logits = torch.full((B * 8,), float("nan"), device="cuda")
                tok = torch.full((B,), -7, dtype=torch.int32, device="cuda")
                fd, ad = torch.from_numpy(forced).cuda(), torch.from_numpy(active).cuda()
                ld, frd = torch.from_numpy(lens.copy()).cuda(), torch.from_numpy(frame.copy()).cuda()
                L.check(lib.vv_llm_tail_batch(C.byref(m), hd.data_ptr(), hidden, B, out.data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(),
                                              logits.data_ptr(), tok.data_ptr(), fd.data_ptr(), ld.data_ptr(), tok_start, tok_diff, frd.data_ptr(),
                                              ad.data_ptr(), None), "vv_llm_tail_batch")
                torch.cuda.synchronize()
                o, lg, tk = out.cpu().numpy(), logits.cpu().numpy().reshape(B, 8), tok.cpu().numpy()
                ln, fr = ld.cpu().numpy(), frd.cpu().numpy()
                for b in range(B):
                    ro, rl, rt, rlens, rfr = _ref_tail(h[2 * b: 2 * b + 2].numpy(), norm_w.cpu().numpy(), wn, ids, int(forced[b]),
                                                       lens[2 * b: 2 * b + 2], int(frame[b]), int(active[b]), tok_start, tok_diff)
                    worst_row = max(worst_row, float(np.abs(o[2 * b: 2 * b + 2] - ro).max() / np.abs(ro).max()))
                    worst_lg = max(worst_lg, float((np.abs(lg[b, :nv] - rl) / _ref_tail.scale).max()))
                    srt = np.sort(rl)
                    if forced[b] < 0 and nv > 1 and srt[-1] - srt[-2] < 1e-5 * max(1.0, abs(srt[-1])):
                        # a near-tie that fp32 rounding may decide either way: the rule is then checked on the kernel's own logits
                        l32 = lg[b, :nv]
                        rt = int(ids[np.flatnonzero(l32 == l32.max())].min())
                    assert int(tk[b]) == rt, (B, nv, ts_mode, b)
                    assert ln[2 * b: 2 * b + 2].tolist() == rlens, (B, nv, ts_mode, b, active[b])
                    assert int(fr[b]) == rfr, (B, nv, ts_mode, b)
                    n_checked += 1
    assert worst_row < 1e-5, f"normalised rows: worst relative error {worst_row:.2e}"
    assert worst_lg < 1e-5, f"logits: worst error relative to sum |w||x| {worst_lg:.2e}"
    assert n_checked == 4 * 4 * 10


@pytest.mark.parametrize("kernel", ["batch", "fast", "general"])
def test_llm_tail_ties_pick_smallest_id(lib, kernel):
    """bit-identical w_valid rows give bit-identical logits: the smallest id among them must win, whatever its index"""
    from vibevoice_rocm_amd import _lib as L
    hidden = 512 if kernel != "general" else 510
    nv = 8 if kernel != "general" else 12
    gen = torch.Generator().manual_seed(3)
    norm_w = torch.ones(hidden, device="cuda")
    m = _llm(hidden, L.VV_F32, norm_w)
    base = torch.randn(hidden, generator=gen)
    for trial in range(6):
        w = torch.randn(nv, hidden, generator=gen) * 0.01
        tied = sorted(np.random.default_rng(trial).choice(nv, 3, replace=False).tolist())
        for i in tied:
            w[i] = base
        ids = np.random.default_rng(10 + trial).permutation(np.arange(200, 200 + nv)).astype(np.int32)
        h = base.repeat(2, 1).contiguous().cuda()           # row 0 aligned with the tied rows: they hold the maximum
        out = torch.empty(2, hidden, device="cuda")
        logits = torch.empty(16, device="cuda")
        tok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
        wd, idd = w.cuda(), torch.from_numpy(ids).cuda()
        if kernel == "batch":
            rc = lib.vv_llm_tail_batch(C.byref(m), h.data_ptr(), hidden, 1, out.data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(),
                                       logits.data_ptr(), tok.data_ptr(), None, None, 0, 0, None, None, None)
        else:
            rc = lib.vv_llm_tail(C.byref(m), h.data_ptr(), hidden, 2, out.data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(),
                                 logits.data_ptr(), tok.data_ptr(), None, None, 0, 0, None, None)
        L.check(rc, kernel)
        torch.cuda.synchronize()
        lg = logits.cpu().numpy()[:nv]
        assert len({float(lg[i]) for i in tied}) == 1 and lg[tied[0]] == lg.max(), (trial, lg)
        assert int(tok.item()) == min(int(ids[i]) for i in tied), (kernel, trial, ids[tied].tolist(), int(tok.item()))


def _tail_is_fast(R, nv, hidden, ldh, ldo, h_ptr, out_ptr, w_ptr, bf16):
    """the dispatch condition of vv_llm_tail (vv_fused.hip) restated: True = llm_tail_fast_kernel, False = the general LDS kernel"""
    return (R <= 2 and nv <= 8 and hidden % 4 == 0 and hidden <= 4096 and h_ptr % 16 == 0 and ldh % 4 == 0 and out_ptr % 16 == 0
            and ldo % 4 == 0 and w_ptr % (8 if bf16 else 16) == 0)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("R,nv,hidden,ldh_pad,fast", [(1, 4, 512, 0, True), (2, 8, 1536, 0, True), (2, 5, 4096, 0, True),
                                                     (3, 5, 512, 0, False), (5, 9, 1536, 1, False), (2, 16, 514, 3, False),
                                                     (3, 16, 67, 0, False), (1, 4, 510, 1, False)])
def test_llm_tail_vs_fp64(lib, bf16, R, nv, hidden, ldh_pad, fast):
    """vv_llm_tail, both kernels: R rows normalised (all of them), logits of row 0, first maximum / forced, bookkeeping.  Which kernel
    ran is read off the dispatch condition (the `fast` column is asserted against it), not timed."""
    from vibevoice_rocm_amd import _lib as L
    gen = torch.Generator().manual_seed(R * 100 + nv + hidden)
    rng = np.random.default_rng(R + nv + hidden)
    norm_w = (1 + 0.1 * torch.randn(hidden, generator=gen)).cuda()
    m = _llm(hidden, L.VV_BF16 if bf16 else L.VV_F32, norm_w)
    ldh = hidden + ldh_pad                                   # odd ldh_pad: an odd row stride, misaligned rows
    w, wn = _w_valid(nv, hidden, bf16, gen)
    wd = w.cuda()
    ids = rng.permutation(np.arange(300, 300 + nv)).astype(np.int32)
    idd = torch.from_numpy(ids).cuda()
    for case in range(4):
        hbuf = torch.randn(R, ldh, generator=gen) * 2
        hd = hbuf.cuda()
        out = torch.full((R, hidden), float("nan"), device="cuda")
        assert _tail_is_fast(R, nv, hidden, ldh, hidden, hd.data_ptr(), out.data_ptr(), wd.data_ptr(), bf16) == fast
        forced = -1 if case % 2 == 0 else int(ids[-1])
        tok_start, tok_diff = [(-1, int(ids[0])), (int(ids[-1]), int(ids[0])), (5, 6), (int(ids[1 % nv]), int(ids[-1]))][case]
        lens = rng.integers(1, 40, 2).astype(np.int32)
        frame = int(rng.integers(0, 5))
        logits = torch.full((16,), float("nan"), device="cuda")
        tok = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        fd = torch.tensor([forced], dtype=torch.int32, device="cuda")
        ld, frd = torch.from_numpy(lens.copy()).cuda(), torch.tensor([frame], dtype=torch.int32, device="cuda")
        L.check(lib.vv_llm_tail(C.byref(m), hd.data_ptr(), ldh, R, out.data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(), logits.data_ptr(),
                                tok.data_ptr(), fd.data_ptr(), ld.data_ptr(), tok_start, tok_diff, frd.data_ptr(), None), "vv_llm_tail")
        torch.cuda.synchronize()
        hn = hbuf[:, :hidden].numpy()
        ro, rl, rt, rlens, rfr = _ref_tail(hn[:2] if R >= 2 else hn, norm_w.cpu().numpy(), wn, ids, forced, lens, frame, 1, tok_start, tok_diff)
        ro_all = hn.astype(np.float64) / np.sqrt(np.mean(hn.astype(np.float64) ** 2, axis=1, keepdims=True) + 1e-6) * norm_w.cpu().numpy()
        o = out.cpu().numpy()
        assert np.abs(o - ro_all).max() / np.abs(ro_all).max() < 1e-5, (case, "rows")
        lg = logits.cpu().numpy()[:nv]
        assert (np.abs(lg - rl) / _ref_tail.scale).max() < 1e-5, (case, lg, rl)
        assert int(tok.item()) == rt, (case, int(tok.item()), rt)
        assert ld.cpu().numpy().tolist() == rlens, (case,)
        assert int(frd.item()) == rfr, (case,)


def test_advance_lens_and_argmax_ids_every_branch(lib):
    from vibevoice_rocm_amd import _lib as L
    ST, SD = 11, 12
    cases = [(ST, ST, SD), (SD, ST, SD), (13, ST, SD), (SD, -1, SD), (13, -1, SD)]
    for t, ts, td in cases:
        for with_frame in (True, False):
            lens = torch.tensor([7, 3], dtype=torch.int32, device="cuda")
            frame = torch.tensor([4], dtype=torch.int32, device="cuda")
            tok = torch.tensor([t], dtype=torch.int32, device="cuda")
            L.check(lib.vv_advance_lens(lens.data_ptr(), tok.data_ptr(), ts, td, frame.data_ptr() if with_frame else None, None), "vv_advance_lens")
            torch.cuda.synchronize()
            _, _, _, rl, rf = _ref_tail(np.ones((2, 4)), np.ones(4), np.ones((1, 4)), [t], t, [7, 3], 4, 1, ts, td)
            assert lens.cpu().tolist() == rl, (t, ts, td)
            assert int(frame.item()) == (rf if with_frame else 4), (t, ts, td, with_frame)
    rng = np.random.default_rng(0)
    for n in (1, 2, 5, 16, 40):
        for trial in range(5):
            lg = rng.standard_normal(n).astype(np.float32)
            if n > 2 and trial >= 2:
                lg[rng.choice(n, min(n, 3), replace=False)] = lg.max() + 1.0      # a tie for the maximum
            ids = rng.permutation(np.arange(50, 50 + n)).astype(np.int32)
            for forced in (None, -1, int(ids[0])):
                tok = torch.full((1,), -7, dtype=torch.int32, device="cuda")
                fd = None if forced is None else torch.tensor([forced], dtype=torch.int32, device="cuda")
                lgd, idd = torch.from_numpy(lg).cuda(), torch.from_numpy(ids).cuda()       # held: the launch is asynchronous
                L.check(lib.vv_argmax_ids(lgd.data_ptr(), n, idd.data_ptr(), tok.data_ptr(), None if fd is None else fd.data_ptr(), None),
                        "vv_argmax_ids")
                torch.cuda.synchronize()
                want = int(ids[np.flatnonzero(lg == lg.max())].min())
                if forced is not None and forced >= 0:
                    want = forced
                assert int(tok.item()) == want, (n, trial, forced)
