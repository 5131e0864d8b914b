"""Seeded token draws on the GPU: vv_token_draws against its numpy restatement (tests/token_draw_ref.py), the _rows step tails
(vv_llm_tail_sample_rows, vv_llm_tail_batch_sample_rows) on the fast and the general kernel against the restatement's choice on the kernels' own
logits and against the argmax tails with the chosen token forced, and generate() / open_session() with seeded_tokens: one dialogue draws the same
tokens alone, on a lane, in a row batch, in a session and behind a voice prefix; requests with different warpers share one graph A."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import token_draw_ref as T
from conftest import rel_rms

pytestmark = pytest.mark.gpu

SEEDS = (0, 1, 2 ** 63 + 5)                 # the high word and the sign bit are in use
POSITIONS = (0, 1, 65535, 100000)
Q_BAR = 4 * 1.7e-7                          # four times the worst error measured on MI355X (test_token_draws_vs_restatement); below the cap 2^-20
Q_CAP = 2.0 ** -20
ROWS = [(1.0, 0, 1.0), (0.6, 0, 0.95), (0.95, 2, 1.0), (1.3, 1, 1.0), (1.0, 0, 0.5), (0.8, 3, 0.85)]      # top_k = 1 and top_p = 0.5 among them
MARGIN, SKIP_CAP = 1 + 1e-4, 0.01


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    lb = L.load()
    L.check(lb.vv_init(), "vv_init")
    return lb


def _i64(seeds):
    return torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64)


def _sampler_rows(rows):
    """[..., 3] fp32 tensor holding vv_sampler rows {float temperature, int top_k, float top_p}"""
    t = torch.tensor([[r[0], 0.0, r[2]] for r in rows], dtype=torch.float32)
    t.view(torch.int32)[:, 1] = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    return t


def test_token_draws_vs_restatement(lib):
    """vv_token_draws for B = 1..4, nv = 1, 4, 5, 8, positions 0 / 1 / 65 535 / 100 000, seeds 0 / 1 / 2^63 + 5, ld_pos 1 and 2, pos_bias 0 and -1
    (position 0 with bias -1 wraps to 2^32 - 1, as the counter word does), ldq 8 and 11 with NaN in the gaps, which must survive.  q against the
    fp64 -ln of the same float32 u: the worst relative error measured on MI355X is 1.7e-7 (1.689e-07 over the 128 calls; profiles/token_seed.txt); the bar is four times that,
    capped at 2^-20 - logf is accurate to a few ulp and nothing else rounds.  The committed clamp triple (u == 1) gives exactly 2^-126."""
    from vibevoice_rocm_amd import _lib as L
    worst, n = 0.0, 0
    for B in (1, 2, 3, 4):
        for nv in (1, 4, 5, 8):
            for ld_pos in (1, 2):
                for bias in (0, -1):
                    for ldq in (8, 11):
                        n += 1
                        seeds = [SEEDS[(b + n) % 3] for b in range(B)]
                        pos = [POSITIONS[(b + n // 3) % 4] for b in range(B)]
                        pd = torch.full((B * ld_pos,), -12345, dtype=torch.int32)
                        pd[::ld_pos] = torch.tensor(pos, dtype=torch.int32)
                        pd, sd = pd.cuda(), _i64(seeds).cuda()
                        q = torch.full((B, ldq), float("nan"), device="cuda")
                        L.check(lib.vv_token_draws(q.data_ptr(), ldq, B, nv, sd.data_ptr(), pd.data_ptr(), ld_pos, bias, None), "vv_token_draws")
                        got = q.cpu().numpy()
                        assert np.isnan(got[:, nv:]).all(), (B, nv, ldq)
                        want = np.stack([T.draws(s, p + bias, nv) for s, p in zip(seeds, pos)])
                        rel = np.abs(got[:, :nv].astype(np.float64) - want) / want
                        worst = max(worst, float(rel.max()))
                        assert (got[:, :nv] > 0).all()
    print(f"vv_token_draws: worst relative error of q against the fp64 -ln of the same u: {worst:.3e} over {n} calls")
    assert worst < Q_BAR <= Q_CAP, worst
    seed, pos, e = T.CLAMP_TRIPLE
    sd, pd = _i64([seed]).cuda(), torch.tensor([pos + 1], dtype=torch.int32).cuda()
    q = torch.zeros(8, device="cuda")
    L.check(lib.vv_token_draws(q.data_ptr(), 8, 1, 8, sd.data_ptr(), pd.data_ptr(), 1, -1, None), "vv_token_draws")
    got = q.cpu().numpy()
    assert got[e] == np.float32(2.0 ** -126), got
    assert np.abs(np.delete(got, e).astype(np.float64) / np.delete(T.draws(seed, pos, 8), e) - 1).max() < Q_BAR


def test_token_draws_rejects_bad_arguments(lib):
    q, sd, pd = torch.full((16,), 7.0, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    a = (q.data_ptr(), 8, 1, 4, sd.data_ptr(), pd.data_ptr(), 1, 0)
    for i, bad in ((0, None), (4, None), (5, None), (2, 0), (3, 0), (3, 9), (1, 3), (6, -1)):
        args = list(a)
        args[i] = bad
        assert lib.vv_token_draws(*args, None) == -1, (i, bad)
    torch.cuda.synchronize()
    assert bool((q == 7.0).all())


def _llm(hidden, wdt, norm_w, eps=1e-6):
    from vibevoice_rocm_amd import _lib as L
    m = L.Llm()
    m.wdt, m.hidden, m.rms_eps, m.final_norm = wdt, hidden, eps, norm_w.data_ptr()
    return m


def _tail_is_fast(nv, hidden, ldh, ldo, h_ptr, out_ptr, w_ptr, bf16):
    """the dispatch condition of vv_llm_tail(_sample / _sample_rows) restated for R <= 2"""
    return (nv <= 8 and hidden % 4 == 0 and hidden <= 4096 and h_ptr % 16 == 0 and ldh % 4 == 0 and out_ptr % 16 == 0 and ldo % 4 == 0
            and w_ptr % (8 if bf16 else 16) == 0)


def _draws_dev(lib, seeds_dev, pos_dev, nv, ld_pos):
    """vv_token_draws for every (seed, position) of the case table: [N, 8] on the host"""
    from vibevoice_rocm_amd import _lib as L
    N = seeds_dev.numel()
    q = torch.ones(N, 8, device="cuda")
    L.check(lib.vv_token_draws(q.data_ptr(), 8, N, nv, seeds_dev.data_ptr(), pos_dev.data_ptr(), ld_pos, 0, None), "vv_token_draws")
    return q.cpu().numpy()


N_CASES = 304


@pytest.mark.parametrize("hidden,ldh_pad,fast,bf16,nv", [(64, 0, True, False, 5), (1536, 0, True, True, 4), (64, 1, False, False, 4), (64, 1, False, True, 5)])
def test_llm_tail_sample_rows(lib, hidden, ldh_pad, fast, bf16, nv):
    """vv_llm_tail_sample_rows, R = 2, on the fast kernel (aligned rows: hidden 64 fp32, hidden 1536 bf16) and the general one (hidden 64, odd row
    stride): 304 (h, position, seed, sampler row) cases, logits of scale ~2, rows with top_k = 1 and top_p = 0.5, every eighth row greedy
    (temperature 0) and every sixteenth with temperature 1e30 - all p equal, so the token is ids[argmin q] and reads the tail's own q.  The token
    equals the restatement's choice on the kernel's own logits_out and vv_token_draws' q wherever its margin is at least 1 + 1e-4 (at most 1 % of
    the cases may be left out); a greedy row equals vv_llm_tail's token exactly; out, logits_out, lens, frame_counter are bit-identical to
    vv_llm_tail with the chosen token forced."""
    from vibevoice_rocm_amd import _lib as L
    gen = torch.Generator().manual_seed(3 * hidden + nv + bf16 + ldh_pad)
    rng = np.random.default_rng(hidden + nv + 2 * bf16 + ldh_pad)
    N = N_CASES
    norm_w = (1 + 0.1 * torch.randn(hidden, generator=gen)).cuda()
    m = _llm(hidden, L.VV_BF16 if bf16 else L.VV_F32, norm_w)
    ldh = hidden + ldh_pad
    w = 2 * torch.randn(nv, hidden, generator=gen) / np.sqrt(hidden)
    wd = (w.to(torch.bfloat16) if bf16 else w).cuda()
    ids = rng.permutation(np.arange(300, 300 + nv)).astype(np.int32)
    idd = torch.from_numpy(ids).cuda()
    rows = [(0.0, 0, 1.0) if n % 8 == 3 else ((1e30, 0, 1.0) if n % 16 == 5 else ROWS[n % len(ROWS)]) for n in range(N)]
    smp = _sampler_rows(rows).cuda()
    seeds = [SEEDS[n % 3] if n % 5 == 0 else int(rng.integers(0, 2 ** 63)) * 2 + int(n & 1) for n in range(N)]
    sd = _i64(seeds).cuda()
    H = torch.randn(N, 2, ldh, generator=gen).cuda()
    pos = rng.integers(1, 4000, (N, 2)).astype(np.int32)
    pos[::7, 0] = [POSITIONS[i % 4] for i in range(len(pos[::7]))]
    lens0 = torch.from_numpy(pos).cuda()
    frame0 = torch.from_numpy(rng.integers(0, 5, N).astype(np.int32)).cuda()
    none = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    res = {}
    for form in ("rows", "forced", "argmax"):
        out = torch.full((N, 2, hidden), float("nan"), device="cuda")
        logits = torch.full((N, 8), float("nan"), device="cuda")
        tok = torch.full((N,), -7, dtype=torch.int32, device="cuda")
        lens, frame = lens0.clone(), frame0.clone()
        for n in range(N):
            assert _tail_is_fast(nv, hidden, ldh, hidden, H[n].data_ptr(), out[n].data_ptr(), wd.data_ptr(), bf16) == fast
            ts, td = int(ids[n % nv]), int(ids[(n + 1) % nv])
            a = (C.byref(m), H[n].data_ptr(), ldh, 2, out[n].data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(), logits[n].data_ptr(), tok[n:].data_ptr())
            if form == "rows":
                L.check(lib.vv_llm_tail_sample_rows(*a, none.data_ptr(), lens[n].data_ptr(), ts, td, frame[n:].data_ptr(), smp[n].data_ptr(), sd[n:].data_ptr(),
                                                    None), "vv_llm_tail_sample_rows")
            else:
                f = res["rows"][2][n:].data_ptr() if form == "forced" else none.data_ptr()
                L.check(lib.vv_llm_tail(*a, f, lens[n].data_ptr(), ts, td, frame[n:].data_ptr(), None), "vv_llm_tail")
        torch.cuda.synchronize()
        res[form] = (out, logits, tok, lens, frame)
    for a, b, what in zip(res["rows"], res["forced"], ("out", "logits_out", "token", "lens", "frame_counter")):
        assert torch.equal(a[:, :nv] if what == "logits_out" else a, b[:, :nv] if what == "logits_out" else b), what
    assert bool((res["rows"][3][:, 0] == lens0[:, 0] + 1).all())
    lg, tk, greedy_tk = res["rows"][1].cpu().numpy()[:, :nv], res["rows"][2].cpu().numpy(), res["argmax"][2].cpu().numpy()
    qd = _draws_dev(lib, sd, lens0, nv, 2)
    assert np.abs(qd[:, :nv].astype(np.float64) / np.stack([T.draws(s, int(p), nv) for s, p in zip(seeds, pos[:, 0])]) - 1).max() < Q_CAP
    skipped, smallest = 0, float("inf")
    for n in range(N):
        if rows[n][0] == 0.0:
            assert tk[n] == greedy_tk[n], n
            continue
        if rows[n][0] == 1e30:
            assert tk[n] == ids[int(np.argmin(qd[n, :nv]))], (n, qd[n], tk[n])
        i, margin = T.choice(lg[n], qd[n, :nv], rows[n], ids)
        smallest = min(smallest, margin)
        if margin < MARGIN:
            skipped += 1
            continue
        assert tk[n] == ids[i], (n, rows[n], lg[n], qd[n], int(tk[n]), int(ids[i]))
    print(f"hidden {hidden} fast {fast} bf16 {bf16}: {skipped} of {N} cases left out, smallest margin {smallest:.6f}")
    assert skipped <= SKIP_CAP * N, skipped
    assert len(set(tk.tolist())) == nv


def test_llm_tail_batch_sample_rows(lib):
    """vv_llm_tail_batch_sample_rows, B = 3 (hidden 1536, bf16, nv 5), 304 cases: dialogue 0 draws under its own row, dialogue 1 is greedy
    (temperature 0), dialogue 2 is in turn inactive (draws, positions stay) or forced; every dialogue has its own seed and position.  Tokens
    against the restatement on the kernel's logits; the greedy dialogue equals vv_llm_tail_batch's token exactly; everything bit-identical to
    vv_llm_tail_batch with the tokens forced.  The batched entry has the fast kernel only: an odd row stride is VV_E_UNSUPPORTED, as it is for
    vv_llm_tail_batch_sample."""
    from vibevoice_rocm_amd import _lib as L
    hidden, nv, B, N = 1536, 5, 3, N_CASES
    gen = torch.Generator().manual_seed(92)
    rng = np.random.default_rng(92)
    norm_w = (1 + 0.1 * torch.randn(hidden, generator=gen)).cuda()
    m = _llm(hidden, L.VV_BF16, norm_w)
    wd = (2 * torch.randn(nv, hidden, generator=gen) / np.sqrt(hidden)).to(torch.bfloat16).cuda()
    ids = rng.permutation(np.arange(500, 500 + nv)).astype(np.int32)
    idd = torch.from_numpy(ids).cuda()
    rows = [[ROWS[n % len(ROWS)], (0.0, 0, 1.0), ROWS[(n + 2) % len(ROWS)]] for n in range(N)]
    smp = torch.stack([_sampler_rows(r) for r in rows]).cuda()
    seeds = [[SEEDS[(n + b) % 3] if n % 4 == 0 else int(rng.integers(0, 2 ** 63)) * 2 + 1 for b in range(B)] for n in range(N)]
    sd = torch.stack([_i64(s) for s in seeds]).cuda()
    H = torch.randn(N, 2 * B, hidden, generator=gen).cuda()
    pos = rng.integers(1, 4000, (N, 2 * B)).astype(np.int32)
    pos[::9, 0] = [POSITIONS[i % 4] for i in range(len(pos[::9]))]
    lens0 = torch.from_numpy(pos).cuda()
    frame0 = torch.from_numpy(rng.integers(0, 5, (N, B)).astype(np.int32)).cuda()
    forced = torch.full((N, B), -1, dtype=torch.int32)
    forced[1::2, 2] = torch.from_numpy(rng.choice(ids, N // 2).astype(np.int32))
    fd = forced.cuda()
    act = torch.ones(N, B, dtype=torch.int32)
    act[0::2, 2] = 0
    actd = act.cuda()
    res = {}
    for form in ("rows", "forced", "argmax"):
        out = torch.full((N, 2 * B, hidden), float("nan"), device="cuda")
        logits = torch.full((N, B, 8), float("nan"), device="cuda")
        tok = torch.full((N, B), -7, dtype=torch.int32, device="cuda")
        lens, frame = lens0.clone(), frame0.clone()
        for n in range(N):
            ts, td = int(ids[n % nv]), int(ids[(n + 1) % nv])
            a = (C.byref(m), H[n].data_ptr(), hidden, B, out[n].data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(), logits[n].data_ptr(), tok[n].data_ptr())
            b = (lens[n].data_ptr(), ts, td, frame[n].data_ptr(), actd[n].data_ptr())
            if form == "rows":
                L.check(lib.vv_llm_tail_batch_sample_rows(*a, fd[n].data_ptr(), *b, smp[n].data_ptr(), sd[n].data_ptr(), None), "vv_llm_tail_batch_sample_rows")
            else:
                f = res["rows"][2][n].data_ptr() if form == "forced" else fd[n].data_ptr()
                L.check(lib.vv_llm_tail_batch(*a, f, *b, None), "vv_llm_tail_batch")
        torch.cuda.synchronize()
        res[form] = (out, logits, tok, lens, frame)
    for a, b, what in zip(res["rows"], res["forced"], ("out", "logits_out", "token", "lens", "frame_counter")):
        assert torch.equal(a[..., :nv] if what == "logits_out" else a, b[..., :nv] if what == "logits_out" else b), what
    lg, tk, greedy_tk = res["rows"][1].cpu().numpy(), res["rows"][2].cpu().numpy(), res["argmax"][2].cpu().numpy()
    lens1 = res["rows"][3].cpu().numpy()
    assert (tk[1::2, 2] == forced[1::2, 2].numpy()).all()                         # the forced dialogue keeps its token
    assert (lens1[0::2, 4:6] == pos[0::2, 4:6]).all() and (lens1[:, 0] == pos[:, 0] + 1).all() and (lens1[:, 2] == pos[:, 2] + 1).all()     # inactive: positions stay
    assert (tk[:, 1] == greedy_tk[:, 1]).all()                                     # the greedy row is vv_llm_tail_batch's argmax
    qd = _draws_dev(lib, sd.reshape(-1), lens0.reshape(-1), nv, 2).reshape(N, B, 8)
    skipped, smallest, checked = 0, float("inf"), 0
    for n in range(N):
        for b in (0, 2):
            if forced[n, b] >= 0:
                continue
            i, margin = T.choice(lg[n, b, :nv], qd[n, b, :nv], rows[n][b], ids)
            smallest, checked = min(smallest, margin), checked + 1
            if margin < MARGIN:
                skipped += 1
                continue
            assert tk[n, b] == ids[i], (n, b, rows[n][b])
    print(f"batch: {skipped} of {checked} choices left out, smallest margin {smallest:.6f}")
    assert skipped <= SKIP_CAP * checked, skipped
    Hodd = torch.randn(2 * B, hidden + 1, device="cuda")
    rc = lib.vv_llm_tail_batch_sample_rows(C.byref(m), Hodd.data_ptr(), hidden + 1, B, res["rows"][0][0].data_ptr(), hidden, wd.data_ptr(), nv, idd.data_ptr(),
                                           res["rows"][1][0].data_ptr(), res["rows"][2][0].data_ptr(), None, lens0[0].clone().data_ptr(), 0, 0, None, None,
                                           smp[0].data_ptr(), sd[0].data_ptr(), None)
    assert rc == -3, rc          # VV_E_UNSUPPORTED


def test_rows_entries_reject_bad_arguments(lib):
    """NULL lens, NULL samplers, NULL seeds, nv > 8: VV_E_ARG from both entries, nothing launched (the outputs keep their fill)"""
    from vibevoice_rocm_amd import _lib as L
    hidden = 64
    norm_w = torch.ones(hidden, device="cuda")
    m = _llm(hidden, L.VV_F32, norm_w)
    h, out, w = torch.zeros(6, hidden, device="cuda"), torch.full((6, hidden), 5.0, device="cuda"), torch.zeros(9, hidden, device="cuda")
    ids = torch.arange(9, dtype=torch.int32, device="cuda")
    lg, tok = torch.full((32,), 5.0, device="cuda"), torch.full((4,), 5, dtype=torch.int32, device="cuda")
    lens, smp, sd = torch.ones(6, dtype=torch.int32, device="cuda"), _sampler_rows([(1.0, 0, 1.0)] * 3).cuda(), torch.zeros(3, dtype=torch.int64, device="cuda")
    for nv, lp, sp, dp in ((4, None, smp.data_ptr(), sd.data_ptr()), (4, lens.data_ptr(), None, sd.data_ptr()), (4, lens.data_ptr(), smp.data_ptr(), None),
                           (9, lens.data_ptr(), smp.data_ptr(), sd.data_ptr())):
        rcs = [lib.vv_llm_tail_sample_rows(C.byref(m), h.data_ptr(), hidden, 2, out.data_ptr(), hidden, w.data_ptr(), nv, ids.data_ptr(), lg.data_ptr(),
                                           tok.data_ptr(), None, lp, 0, 0, None, sp, dp, None),
               lib.vv_llm_tail_batch_sample_rows(C.byref(m), h.data_ptr(), hidden, 3, out.data_ptr(), hidden, w.data_ptr(), nv, ids.data_ptr(), lg.data_ptr(),
                                                 tok.data_ptr(), None, lp, 0, 0, None, None, sp, dp, None)]
        assert rcs == [-1, -1], (nv, rcs)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and bool((lg == 5.0).all()) and bool((tok == 5).all()) and bool((lens == 1).all())


# ---------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------
# One dialogue - a voice prompt of three frames inside a 60-token head, a 25-token suffix (tests/test_hip_voice_prefix.py's inputs) - sampled at
# temperature 1, top_p 0.95 from TOKEN_SEED, its diffusion noise from NOISE_SEED.  The seeds were picked so that the restatement's margin on the
# logits recorded from the dialogue alone is at least 1 + 1e-2 at every step (asserted): the paths' logits differ by the rounding of their GEMVs.
GEN = {"do_sample": True, "temperature": 1.0, "top_p": 0.95}
TOKEN_SEED, NOISE_SEED, NEW_TOKENS = 12, 40, 14         # seed 12 draws ST SE SD SD EOS here, smallest margin 1.21 (seeds 0 .. 23 were tried)
E2E_MARGIN = 1 + 1e-2


def _keys(graphs, name):
    return [k for k in graphs if k[0] == name]


@pytest.fixture(scope="module")
def e2e():
    """the `mid` bf16 model, the dialogue's inputs and the run of the dialogue alone with every step's (position, logits) recorded"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from test_hip_voice_prefix import _inputs
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg = VVConfig.preset("mid")
    m = VibeVoiceForConditionalGenerationInference.from_synthetic(cfg, seed=1234, device="cuda:0", torch_dtype=torch.bfloat16)
    m.set_ddpm_inference_steps(5)
    d = _inputs(cfg)
    ids = torch.cat([d["pre"], d["suffix"][0]])
    mask = torch.cat([d["pre_mask"], torch.zeros(len(d["suffix"][0]), dtype=torch.bool)])
    base = dict(tokenizer=d["tok"], max_new_tokens=NEW_TOKENS, device_noise=True)
    voice = dict(speech_tensors=d["wav"], speech_masks=d["sm"], speech_noise=d["speech_noise"])
    rec = []
    real = {n: getattr(Engine, n) for n in ("first_token", "step_decode", "step_decode_speculative")}

    def spy(name):
        def f(self, *a, **k):
            tok = real[name](self, *a, **k)
            rec.append((int(self.lens[0].item()) - 1, self.logits.cpu().numpy()[: len(self.valid_ids)].copy(), tok))
            return tok
        return f
    for n in real:
        setattr(Engine, n, spy(n))
    try:
        state = torch.get_rng_state()
        alone = m.generate(input_ids=ids[None], speech_input_mask=mask[None], cfg_scale=2.0, generation_config=GEN, seeded_tokens=True,
                           token_seed=TOKEN_SEED, noise_seed=NOISE_SEED, **voice, **base)
        untouched = torch.equal(torch.get_rng_state(), state)
    finally:
        for n in real:
            setattr(Engine, n, real[n])
    S = dict(m=m, cfg=cfg, d=d, ids=ids, mask=mask, base=base, voice=voice, alone=alone, rec=rec, untouched=untouched,
             keys_alone=sorted(k[0] for k in m.engine._graphs))
    yield S
    torch.cuda.synchronize()
    m.release_lanes()
    del m, S
    gc.collect()


def _new_tokens(out, b, L):
    return out.sequences[b, L:].tolist()


def _wav(out, b=0):
    return out.speech_outputs[b][0].float().cpu().numpy()


def test_alone_follows_the_restatement(e2e):
    """The dialogue alone: every step's token is the restatement's choice for (TOKEN_SEED, the position of the token whose hidden state gave the
    logits, the recorded logits) - the first token at the last prompt position, every later one at the position the step wrote - and the
    restatement's margin is at least 1 + 1e-2 at every step, which is what lets the other paths be held to the same tokens.  One "Ar" graph, no
    "AS", no "A"; the CPU generator is untouched (both seeds given); a repeated call repeats the tokens."""
    m, ids, rec = e2e["m"], e2e["ids"], e2e["rec"]
    L0 = len(ids)
    seq = _new_tokens(e2e["alone"], 0, L0)
    valid = sorted({m.config.vocab - 4, m.config.vocab - 3, m.config.vocab - 2, m.config.vocab - 1})
    row = (1.0, 0, 0.95)
    assert len(rec) == len(seq) and [r[0] for r in rec] == list(range(L0 - 1, L0 - 1 + len(seq)))
    margins = []
    for (p, lg, tok), s in zip(rec, seq):
        i, margin = T.choice(lg, T.draws(TOKEN_SEED, p, len(lg)).astype(np.float32), row, valid)
        margins.append(margin)
        assert tok == s == valid[i], (p, lg, tok, valid[i])
    print("alone:", seq, "smallest margin", min(margins))
    assert min(margins) >= E2E_MARGIN, margins
    assert len(set(seq)) >= 3 and (m.config.vocab - 2) in seq           # a sampled stream, with frames in it
    assert e2e["keys_alone"].count("Ar") == 1 and "AS" not in e2e["keys_alone"] and "A" not in e2e["keys_alone"]
    assert e2e["untouched"]
    again = m.generate(input_ids=ids[None], speech_input_mask=e2e["mask"][None], cfg_scale=2.0, generation_config=GEN, seeded_tokens=True,
                       token_seed=TOKEN_SEED, noise_seed=NOISE_SEED, **e2e["voice"], **e2e["base"])
    assert again.sequences.tolist() == e2e["alone"].sequences.tolist() and torch.equal(again.speech_outputs[0], e2e["alone"].speech_outputs[0])
    other = m.generate(input_ids=ids[None], speech_input_mask=e2e["mask"][None], cfg_scale=2.0, generation_config=GEN, seeded_tokens=True,
                       token_seed=TOKEN_SEED + 1, noise_seed=NOISE_SEED, **e2e["voice"], **e2e["base"])
    assert other.sequences.tolist() != e2e["alone"].sequences.tolist()


def _batch_of_three(e2e, where):
    """the dialogue as number `where` of three (the others: plain prompts of 30 and 21 tokens), left-padded as the processor pads"""
    cfg, ids, mask = e2e["cfg"], e2e["ids"], e2e["mask"]
    g = torch.Generator().manual_seed(6)
    others = [torch.cat([torch.randint(1, cfg.vocab - 8, (n - 1,), generator=g), torch.tensor([cfg.vocab - 4])]) for n in (30, 21)]
    prompts = others[:where] + [ids] + others[where:]
    sp = [torch.zeros(len(p), dtype=torch.bool) for p in prompts]
    sp[where] = mask
    Lp = max(len(p) for p in prompts)
    pad = lambda t, v: torch.cat([torch.full((Lp - len(t),), v, dtype=t.dtype), t])
    return (torch.stack([pad(p, 0) for p in prompts]), torch.stack([pad(torch.ones(len(p), dtype=torch.long), 0) for p in prompts]),
            torch.stack([pad(s, False) for s in sp]), Lp)


@pytest.mark.parametrize("row_batch", [False, True])
def test_same_tokens_in_a_batch_of_three(e2e, row_batch):
    """The dialogue as dialogue 1 of a 3-dialogue call, on the lanes and row-batched, token seeds given per dialogue: its tokens are the ones it
    draws alone; waveform against the run alone at 1e-2 (the lanes-vs-row-batch bar of tests/test_hip_rowbatch.py).  The neighbours follow forced
    schedules without a frame: a batched call couples its dialogues where the reference's batched loop does (batchloop._BatchCoupling - a
    neighbour's first frame restarts the others' conv state), which no seed can undo; neighbours that never diffuse leave the dialogue the
    computation it is alone.  The CPU generator is untouched."""
    m, base, V = e2e["m"], e2e["base"], e2e["cfg"].vocab
    ids3, am, sp, Lp = _batch_of_three(e2e, 1)
    cfgs = [{"do_sample": True, "temperature": 0.7, "top_k": 3}, GEN, {"do_sample": False}]
    ST, SE, EOS = V - 4, V - 3, V - 1
    forced = [[ST, SE] * 4 + [EOS], None, [SE, ST] * 8 + [EOS]]
    state = torch.get_rng_state()
    out = m.generate(input_ids=ids3, attention_mask=am, speech_input_mask=sp, cfg_scale=2.0, generation_config=cfgs, seeded_tokens=True,
                     token_seed=[99, TOKEN_SEED, 5], noise_seed=[41, NOISE_SEED, 42], row_batch=row_batch, forced_tokens=forced, **e2e["voice"], **base)
    assert torch.equal(torch.get_rng_state(), state)
    assert ((3, 0) in m._rowbatch) == row_batch
    want = _new_tokens(e2e["alone"], 0, len(e2e["ids"]))
    got = _new_tokens(out, 1, Lp)
    print(f"row_batch {row_batch}: tokens {got}")
    assert got[: len(want)] == want, (got, want)
    err = rel_rms(_wav(out, 1), _wav(e2e["alone"]), what=f"seeded tokens: dialogue in a batch of three (row_batch={row_batch}) vs alone, mid bf16, waveform")
    print(f"row_batch {row_batch}: waveform rel RMS vs alone {err:.3e}")
    assert err < 1e-2, err


def test_mixed_warpers_share_one_graph(e2e):
    """Two dialogues with different warpers and a greedy one, sampled freely in one row batch: ONE graph A - a single ("Ar", ...) key, no
    ("AS", ...), no ("A", ...) - serves all three; the call repeats its tokens when repeated, leaves the CPU generator alone (every seed given)
    and, with token_seed=None, draws its seeds from it after the noise seeds (the noise seeds of a seeded call stay what they were)."""
    m, base = e2e["m"], e2e["base"]
    ids3, am, sp, Lp = _batch_of_three(e2e, 1)
    cfgs = [{"do_sample": True, "temperature": 0.7, "top_k": 3}, GEN, {"do_sample": False}]
    kw = dict(input_ids=ids3, attention_mask=am, speech_input_mask=sp, cfg_scale=[1.3, 2.0, 1.5], generation_config=cfgs, seeded_tokens=True, row_batch=True,
              **e2e["voice"], **base)
    m.generate(**dict(kw, max_new_tokens=2), token_seed=1, noise_seed=1)          # the row batch exists (and has its cfg_rows graphs) before the count
    rb = m._rowbatch[(3, 0)]
    rb._drop_graphs()
    state = torch.get_rng_state()
    a = m.generate(token_seed=[99, TOKEN_SEED, 5], noise_seed=[41, NOISE_SEED, 42], **kw)
    assert torch.equal(torch.get_rng_state(), state)
    graphs = sorted(rb._graphs)
    assert len(_keys(graphs, "Ar")) == 1 and not _keys(graphs, "AS") and not _keys(graphs, "A"), graphs
    b = m.generate(token_seed=[99, TOKEN_SEED, 5], noise_seed=[41, NOISE_SEED, 42], **kw)
    assert a.sequences.tolist() == b.sequences.tolist()
    print("mixed warpers:", [_new_tokens(a, i, Lp) for i in range(3)])
    torch.manual_seed(21)
    want_noise = [int(v) for v in torch.randint(0, 2 ** 62, (3,))]
    want_tok = [int(v) for v in torch.randint(0, 2 ** 62, (3,))]
    after = torch.get_rng_state()
    torch.manual_seed(21)
    c = m.generate(**kw)
    assert torch.equal(torch.get_rng_state(), after)
    d = m.generate(token_seed=want_tok, noise_seed=want_noise, **kw)
    assert c.sequences.tolist() == d.sequences.tolist()


def test_same_tokens_behind_a_voice_prefix(e2e):
    """generate(voice_prefix=): the prefix restores K / V up to the position the full prompt reaches, so the draw indices - and the tokens - are
    the full prompt's; waveform at 2e-2, the prefix-vs-full-prompt bar of tests/test_hip_voice_prefix.py"""
    from test_hip_voice_prefix import _prepare
    m, d = e2e["m"], e2e["d"]
    vp = _prepare(m, d)
    out = m.generate(input_ids=e2e["ids"][None], speech_input_mask=e2e["mask"][None], cfg_scale=2.0, generation_config=GEN, seeded_tokens=True,
                     token_seed=TOKEN_SEED, noise_seed=NOISE_SEED, voice_prefix=vp, **e2e["base"])
    assert out.sequences.tolist() == e2e["alone"].sequences.tolist()
    err = rel_rms(_wav(out), _wav(e2e["alone"]), what="seeded tokens: generate(voice_prefix=) vs the full prompt, mid bf16, waveform")
    assert err < 2e-2, err


def test_same_tokens_in_a_session(e2e):
    """A 2-slot session opened with seeded_tokens: another request (its own warpers) runs first, the dialogue is admitted mid-flight behind it and
    a greedy request queues behind both - the dialogue draws the tokens it draws alone (waveform at 1e-2, the session bar of
    tests/test_hip_session.py), one ("Ar", ...) key serves all three and no ("AS", ...) exists; with both seeds given submit() leaves the CPU
    generator alone.  Without seeded_tokens a session refuses per-request warpers and captures "AS" with its sampler, as before."""
    m, cfg, tok = e2e["m"], e2e["cfg"], e2e["d"]["tok"]
    g = torch.Generator().manual_seed(8)
    other = torch.cat([torch.randint(1, cfg.vocab - 8, (33,), generator=g), torch.tensor([cfg.vocab - 4])])
    for rb in m._rowbatch.values():
        rb._drop_graphs()
    with m.open_session(tokenizer=tok, slots=2, max_context=256, generation_config={"do_sample": True, "temperature": 0.8}, seeded_tokens=True) as sess:
        h0 = sess.submit(input_ids=other[None], cfg_scale=1.3, max_new_tokens=12, noise_seed=1, token_seed=2, forced_tokens=[cfg.vocab - 2] * 6)
        for _ in range(3):
            sess.step()
        assert not h0.done
        state = torch.get_rng_state()
        h1 = sess.submit(input_ids=e2e["ids"][None], speech_input_mask=e2e["mask"][None], cfg_scale=2.0, max_new_tokens=NEW_TOKENS, generation_config=GEN,
                         token_seed=TOKEN_SEED, noise_seed=NOISE_SEED, **e2e["voice"])
        h2 = sess.submit(input_ids=other[None], cfg_scale=1.3, max_new_tokens=6, generation_config={"do_sample": False}, token_seed=3, noise_seed=4)
        assert torch.equal(torch.get_rng_state(), state)
        sess.run()
        graphs = dict(m._rowbatch[(2, 0, "session")]._graphs)
    assert h0.done and h1.done and h2.done and h1.slot == 1
    assert len(_keys(graphs, "Ar")) == 1 and not _keys(graphs, "AS") and not _keys(graphs, "A"), sorted(graphs)
    got = h1.result()
    assert got.sequences.tolist() == e2e["alone"].sequences.tolist()
    err = rel_rms(_wav(got), _wav(e2e["alone"]), what="seeded tokens: dialogue admitted mid-flight into a 2-slot session vs alone, mid bf16, waveform")
    print(f"session: waveform rel RMS vs alone {err:.3e}")
    assert err < 1e-2, err
    for rb in m._rowbatch.values():
        rb._drop_graphs()
    with m.open_session(tokenizer=tok, slots=2, max_context=256, generation_config=GEN, device_sampling=True) as sess:
        with pytest.raises(ValueError):
            sess.submit(input_ids=other[None], generation_config=GEN)
        with pytest.raises(ValueError):
            sess.submit(input_ids=other[None], token_seed=1)
        h = sess.submit(input_ids=other[None], cfg_scale=1.3, max_new_tokens=4, noise_seed=1)
        sess.run()
        graphs = dict(m._rowbatch[(2, 0, "session")]._graphs)
    assert h.done and _keys(graphs, "AS") == [("AS", cfg.vocab - 4, cfg.vocab - 2, 1.0, 0, 0.95)] and not _keys(graphs, "Ar")


def test_no_change_by_default(e2e):
    """seeded_tokens off: generate() captures the graph keys it captured before - "A" greedy, ("AS", ..., warpers) with device sampling - and
    never "Ar"; seeded_tokens=True with do_sample false changes nothing: same keys, bit-identical output, nothing drawn."""
    m, cfg, tok = e2e["m"], e2e["cfg"], e2e["d"]["tok"]
    ids = e2e["ids"]
    ST, SD = cfg.vocab - 4, cfg.vocab - 2
    kw = dict(input_ids=ids[None], tokenizer=tok, cfg_scale=1.3, max_new_tokens=6, device_noise=True, noise_seed=9, forced_tokens=[SD, SD])     # two frames, then free
    m.engine._drop_graphs()
    a = m.generate(**kw)
    keys_greedy = sorted(m.engine._graphs)
    assert _keys(keys_greedy, "A") == [("A", ST, SD)] and not _keys(keys_greedy, "Ar") and not _keys(keys_greedy, "AS")
    state = torch.get_rng_state()
    b = m.generate(seeded_tokens=True, generation_config={"do_sample": False, "temperature": 0.5}, **kw)
    assert torch.equal(torch.get_rng_state(), state) and sorted(m.engine._graphs) == keys_greedy
    assert a.sequences.tolist() == b.sequences.tolist() and a.speech_outputs[0] is not None and torch.equal(a.speech_outputs[0], b.speech_outputs[0])
    torch.manual_seed(3)
    m.generate(generation_config=GEN, device_sampling=True, **kw)
    assert _keys(m.engine._graphs, "AS") == [("AS", ST, SD, 1.0, 0, 0.95)] and not _keys(m.engine._graphs, "Ar")
