"""Seeded token draws, the parts a machine without a GPU can check: the statistics of the draw's definition (tests/token_draw_ref.py, the
restatement the GPU tests hold vv_token_draws and the _rows step tails to), the clamp at u == 1, the separation of the token domain's Philox
counters from the noise's, the C ABI entries, and the host logic - batchloop.run with BatchCall.token_sampling and a seeded-token Session under a
recording driver, generator use, and every refusal of generate() / open_session() / submit()."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

import philox_ref as P
import token_draw_ref as T
from test_host_session import _D, _E, _EOS, _LATENT, _PAD, _SPECIAL, _ST, _Fake, _schedule
from vibevoice_rocm_amd import batchloop
from vibevoice_rocm_amd.batchloop import Session, SessionRequest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the draw's definition
# ---------------------------------------------------------------------------------------------------------------
def _ks(q):
    n = q.size
    s = np.sort(q)
    cdf = 1.0 - np.exp(-s)
    return np.sqrt(n) * max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(n) / n))


def test_draws_are_exponential():
    """2^19 draws (seed 1234, positions 0 .. 65535, 8 each) against Exp(1): Kolmogorov-Smirnov sqrt(n) D < 1.36 (the 5 % point; 1.09 here), mean
    and variance within five standard errors of 1, every q > 0"""
    q = T.draws(1234, np.arange(65536), 8).reshape(-1)
    assert q.size == 2 ** 19 and (q > 0).all() and np.isfinite(q).all()
    ks = _ks(q)
    print(f"mean {q.mean():.4f} var {q.var():.4f} KS {ks:.2f}")
    assert ks < 1.36
    assert abs(q.mean() - 1) < 5 / np.sqrt(q.size) and abs(q.var() - 1) < 5 * np.sqrt(8 / q.size)       # var of (q - 1)^2 for Exp(1) is 8


@pytest.mark.parametrize("seed", [0, 2, 3, 2024])
def test_token_frequencies(seed):
    """argmax p / q over 20 000 positions for logits [1.0, 0.2, -0.5, 0.7, -1.5] at temperature 1: the token frequencies against softmax, chi^2
    with 4 degrees of freedom below 13.28 (the 1 % point; seeds 0, 2, 3, 2024 give 2.9, 1.1, 4.0, 3.7)"""
    l = np.array([1.0, 0.2, -0.5, 0.7, -1.5])
    p = np.exp(l - l.max())
    p /= p.sum()
    N = 20000
    q = T.draws(seed, np.arange(N), 5).astype(np.float32)
    tok = np.argmax(p.astype(np.float32)[None] / q, axis=1)
    cnt = np.bincount(tok, minlength=5)
    chi2 = float(((cnt - N * p) ** 2 / (N * p)).sum())
    print(f"seed {seed}: counts {cnt.tolist()} chi2 {chi2:.2f}")
    assert chi2 < 13.28
    # the restatement's choice() is that argmax (temperature 1, no top-k / top-p) on a sample of the positions
    for n in range(0, N, 997):
        assert T.choice(l.astype(np.float32), q[n], (1.0, 0, 1.0))[0] == tok[n]


def test_neighbouring_seeds_and_positions_are_uncorrelated():
    """correlation of the draws of seed / seed + 1 and of position / position + 1 below 5e-3 in magnitude (2^19 pairs each)"""
    pos = np.arange(65536)
    a, b = T.draws(1234, pos, 8).reshape(-1), T.draws(1235, pos, 8).reshape(-1)
    c_seed = float(np.corrcoef(a, b)[0, 1])
    c_pos = float(np.corrcoef(T.draws(1234, pos, 8).reshape(-1), T.draws(1234, pos + 1, 8).reshape(-1))[0, 1])
    print(f"corr seed/seed+1 {c_seed:.1e}, position/position+1 {c_pos:.1e}")
    assert abs(c_seed) < 5e-3 and abs(c_pos) < 5e-3


def test_token_counters_are_not_noise_counters():
    """every counter of the token domain has fourth word 1; every counter normal_row uses has fourth word 0 (philox_ref.normal_quads) - so for one
    seed no Philox block is shared - and the words really differ where the first three counter words coincide"""
    (j, p, k, w), _ = T.counters(np.arange(100)[:, None], np.arange(8)[None])
    assert w == 1 and k == 0 and set(np.unique(j).tolist()) == {0, 1}
    src = open(os.path.join(ROOT, "tests", "philox_ref.py")).read()
    assert re.search(r"philox4x32_10\(\(j, int\(frame\) & 0xFFFFFFFF, int\(kind\), 0\)", src)       # the noise's layout: (quad, frame, kind, 0)
    seed = 0x0123456789abcdef
    for pos in (0, 7, 65535):
        tok = T.words(seed, pos, 8)
        noise = np.stack(P.philox4x32_10((np.arange(2), pos, 0, 0), (seed & 0xFFFFFFFF, seed >> 32)), axis=-1).reshape(-1)
        assert not (tok == noise).any()
    # element i is word i % 4 of quad i // 4
    x = P.philox4x32_10((1, 9, 0, 1), (5, 0))
    assert [int(v) for v in T.words(5, 9, 8)[4:]] == [int(v) for v in x]


def test_clamp_triple():
    """the committed (seed, position, element): its Philox word is >= 2^32 - 128, converts to 2^32, u == 1.0f, -ln u == 0 and the draw is the
    smallest positive normal float.  It is the first such word of seed 0 (searched from the block that holds it; about one word in 2^25 is)."""
    seed, pos, e = T.CLAMP_TRIPLE
    w = int(T.words(seed, pos, 8)[e])
    assert 2 ** 32 - 128 <= w < 2 ** 32
    assert T.uniforms(seed, pos, 8)[e] == np.float32(1.0)
    q = T.draws(seed, pos, 8)
    assert q[e] == T.TINY == 2.0 ** -126 and (np.delete(q, e) > 1e-9).all()
    blk = 1 << 20
    assert T.find_clamp_triple(seed, blk, first_block=pos // blk, max_blocks=1) == T.CLAMP_TRIPLE
    assert (T.words(seed, np.arange((pos // blk) * blk, pos), 8) < 2 ** 32 - 128).all()


def test_abi_entries():
    from vibevoice_rocm_amd import _lib
    vp, i64 = C.c_void_p, C.c_int64
    assert _lib.PROTOTYPES["vv_token_draws"] == (C.c_int, [vp, i64, C.c_int, C.c_int, vp, vp, i64, C.c_int, vp])
    tail = [C.POINTER(_lib.Llm), vp, i64, C.c_int, vp, i64, vp, C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp]
    assert _lib.PROTOTYPES["vv_llm_tail_sample_rows"] == (C.c_int, tail + [vp, vp, vp])
    assert _lib.PROTOTYPES["vv_llm_tail_batch_sample_rows"] == (C.c_int, tail + [vp, vp, vp, vp])
    lib = _lib.load()
    for name in ("vv_token_draws", "vv_llm_tail_sample_rows", "vv_llm_tail_batch_sample_rows"):
        assert hasattr(lib, name)
    assert lib.vv_abi_version() == 6
    # null pointers are refused before anything touches a device
    assert lib.vv_token_draws(None, 8, 1, 4, None, None, 1, 0, None) == -1


# ---------------------------------------------------------------------------------------------------------------
# host logic under the recording fake
# ---------------------------------------------------------------------------------------------------------------
class _SeededFake(_Fake):
    """test_host_session's recording driver playing the device: a dialogue without a forced token gets the next token of its request's script
    (what the device would draw from its seed and position - a function of the request alone); q and sample_fn must never arrive."""

    def __init__(self, scripts, **kw):
        super().__init__(**kw)
        self.scripts, self.at_step, self.rows, self.calls = scripts, {}, {}, []

    def set_token_sampling(self, samplers, seeds):
        self.calls.append(("set_token_sampling", list(samplers), list(seeds)))
        self.at_step[0] = 0

    def admit(self, b, req):
        super().admit(b, req)
        self.at_step[b] = 0
        self.rows[req.tag] = (req.sampler, req.token_seed)

    def _tok(self, b, forced):
        t = self.scripts[self.who[b]][self.at_step[b]] if forced is None else forced
        self.at_step[b] += 1
        return t

    def first_tokens(self, live, forced, sample_fn, q=None):
        assert q is None and sample_fn is None
        toks = {b: self._tok(b, forced[b]) for b in live}
        for b in live:
            self._rec(b, "first", toks[b])
        return toks

    def decode(self, live, forced, eligible, sample_fn, deliver, q=None):
        assert q is None and sample_fn is None
        assert set(eligible) <= set(live) == set(forced)
        toks = {b: self._tok(b, forced[b]) for b in live}
        for b in live:
            self._rec(b, "decode", toks[b], self._row(eligible[b]) if b in eligible else None)
        deliver()
        return toks, set(eligible)


def _seeded_request(tag, L0, rows, max_length_times):
    req = SessionRequest(prompt=torch.arange(10 + tag, 10 + tag + L0), max_length_times=max_length_times, cfg_scale=1.0 + 0.1 * (tag % 5),
                         noise_seed=7000 + tag, sampler=rows[tag % len(rows)], token_seed=9000 + tag)
    req.tag = tag
    return req


def _alone_seeded(req, script):
    drv = _SeededFake({req.tag: script}, alone=req.tag)
    call = batchloop.BatchCall(special=_SPECIAL, pad_id=_PAD, max_pos=4096, latent=_LATENT, max_length_times=req.max_length_times,
                               noise_seeds=[req.noise_seed], token_sampling=([req.sampler], [req.token_seed]))
    ids = req.prompt[None]
    out = batchloop.run(drv, ids, torch.ones_like(ids), None, None, call)
    assert drv.calls == [("set_token_sampling", [req.sampler], [req.token_seed])]
    return [e[1:] for e in drv.log if e[0] == req.tag], out


def test_seeded_session_equals_alone_and_draws_nothing():
    """Random scripts, 2..6 slots, requests with different sampler rows (greedy among them) arriving mid-flight: every dialogue receives - admit
    aside - the driver calls batchloop.run makes for it alone under BatchCall.token_sampling, and ends with the same sequence; admit carries each
    request's own sampler row and token seed; first_tokens / decode get neither q nor a sample_fn (asserted in the fake); with every seed given
    the CPU generator is never touched."""
    rng = random.Random(5)
    rows = [batchloop.GREEDY_ROW, (1.0, 0, 0.95), (0.7, 2, 1.0), (1.3, 1, 0.5)]
    midflight = 0
    state = torch.get_rng_state()
    for it in range(60):
        slots, n_req = rng.randint(2, 6), rng.randint(4, 12)
        scripts = {tag: _schedule(rng) + [_D] * 60 for tag in range(n_req)}
        reqs = [_seeded_request(tag, rng.randint(3, 9), rows, rng.choice([2, 3, 50] if _EOS in scripts[tag] else [2, 3])) for tag in range(n_req)]
        arrive = sorted(rng.randint(0, 10) for _ in range(n_req))
        drv = _SeededFake(scripts)
        drv.slots = slots
        sess = Session(drv, slots, _SPECIAL, _PAD, 4096, _LATENT, max_context=1024, device_noise=True, sampler=(0.9, 0, 0.9), seeded_tokens=True)
        assert sess.sampler is None and sess.default_row == (0.9, 0, 0.9)
        handles, t = {}, 0
        while True:
            for tag in range(n_req):
                if arrive[tag] == t:
                    handles[tag] = sess.submit(reqs[tag])
            going = sess.step()
            t += 1
            if not going and t > arrive[-1]:
                break
            assert t < 2000
        sess.close()
        for tag, req in enumerate(reqs):
            assert drv.rows[tag] == (rows[tag % len(rows)], 9000 + tag)
            want_log, want = _alone_seeded(req, scripts[tag])
            got_log = [e[1:] for e in drv.log if e[0] == tag]
            assert got_log == want_log, (it, tag, got_log, want_log)
            assert handles[tag].result().sequences.tolist() == want.sequences.tolist()
        first = {tag: next(i for i, e in enumerate(drv.log) if e[0] == tag) for tag in range(n_req)}
        midflight += sum(1 for tag, others in drv.admitted_with if any(e[0] in others and e[1] == "decode" for e in drv.log[:first[tag]]))
    assert torch.equal(torch.get_rng_state(), state)
    assert midflight >= 20, midflight


def test_session_seed_defaults_and_generator_use():
    """submit() in a seeded-token session: sampler None -> the session's row (greedy when the session has none); token_seed None -> one draw from
    the CPU generator, made after the noise seed's - so a seeded device-noise request keeps its noise seed - and none when both are given"""
    drv = _SeededFake({})
    sess = Session(drv, 2, _SPECIAL, _PAD, 4096, _LATENT, max_context=256, device_noise=True, sampler=(0.8, 3, 0.9), seeded_tokens=True)
    torch.manual_seed(11)
    want_noise, want_tok = int(torch.randint(0, 2 ** 62, (1,))), int(torch.randint(0, 2 ** 62, (1,)))
    torch.manual_seed(11)
    r = SessionRequest(prompt=torch.arange(5))
    sess.submit(r)
    assert (r.noise_seed, r.token_seed, r.sampler) == (want_noise, want_tok, (0.8, 3, 0.9))
    torch.manual_seed(11)
    r = SessionRequest(prompt=torch.arange(5), noise_seed=3)
    sess.submit(r)
    assert r.token_seed == want_noise                      # the one draw of this submit
    state = torch.get_rng_state()
    r = SessionRequest(prompt=torch.arange(5), noise_seed=3, token_seed=2 ** 63 + 5, sampler=batchloop.GREEDY_ROW)
    sess.submit(r)
    assert torch.equal(torch.get_rng_state(), state) and r.token_seed == 2 ** 63 + 5 and r.sampler == batchloop.GREEDY_ROW
    greedy = Session(_SeededFake({}), 2, _SPECIAL, _PAD, 4096, _LATENT, max_context=256, seeded_tokens=True)
    assert greedy.default_row == batchloop.GREEDY_ROW
    # today's session is what it was: one sampler, told to the driver once; draws uploaded per step
    told = []
    plain = _Fake()
    plain.set_sampler = lambda *a: told.append(a)
    s2 = Session(plain, 2, _SPECIAL, _PAD, 4096, _LATENT, max_context=256, sampler=(0.8, 3, 0.9))
    assert told == [(0.8, 3, 0.9)] and s2.sampler == (0.8, 3, 0.9) and not s2.seeded_tokens


def test_run_token_sampling_checks():
    """BatchCall.token_sampling: the wrong number of rows or seeds, or a sampler / sample_fn next to it, is a ValueError"""
    ids = torch.arange(4)[None]
    for kw in (dict(token_sampling=([batchloop.GREEDY_ROW] * 2, [1])), dict(token_sampling=([batchloop.GREEDY_ROW], [1, 2])),
               dict(token_sampling=([batchloop.GREEDY_ROW], [1]), sampler=(1.0, 0, 1.0)),
               dict(token_sampling=([batchloop.GREEDY_ROW], [1]), sample_fn=lambda l, i: i[0])):
        call = batchloop.BatchCall(special=_SPECIAL, pad_id=_PAD, max_pos=4096, latent=_LATENT, **kw)
        drv = _SeededFake({0: [_EOS]}, alone=0)
        drv.set_sampler = lambda *a: None
        with pytest.raises(ValueError):
            batchloop.run(drv, ids, torch.ones_like(ids), None, None, call)


def test_sampler_row():
    assert batchloop.sampler_row(None) == batchloop.sampler_row({"do_sample": False, "temperature": 0.5}) == batchloop.GREEDY_ROW == (0.0, 0, 1.0)
    assert batchloop.sampler_row({"do_sample": True, "temperature": 0.7, "top_k": 3, "top_p": 0.9}) == (0.7, 3, 0.9)
    assert batchloop.sampler_row({"do_sample": True}) == (1.0, 0, 1.0)
    for bad in ({"temperature": -1.0}, {"top_p": 1.5}, {"top_p": -0.1}, {"temperature": float("inf")}):
        with pytest.raises(ValueError):
            batchloop.sampler_row(dict(do_sample=True, **bad))


def test_refusals():
    """generate(): a generation_config list without seeded_tokens, a list of the wrong length, token_seed without seeded_tokens, seeded_tokens with
    device_sampling=False given explicitly, a token_seed list of the wrong length - each a ValueError before anything runs (a bare instance shows
    it).  Sessions: per-request generation_config / token_seed without seeded_tokens; seeded_tokens with a host sampler or device_sampling=False."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as Model
    from vibevoice_rocm_amd.modeling import VibeVoiceSession

    class Tok:
        speech_start_id, speech_end_id, speech_diffusion_id, eos_token_id, bos_token_id, pad_id = _ST, _E, _D, _EOS, None, _PAD
    m = object.__new__(Model)
    m._session, m.seeded_tokens, m.device_sampling, m.config = None, False, False, None
    ids = torch.zeros(2, 6, dtype=torch.long)
    g = {"do_sample": True, "temperature": 0.9}
    with pytest.raises(ValueError, match="seeded_tokens"):
        m.generate(input_ids=ids, tokenizer=Tok(), generation_config=[g, g])
    with pytest.raises(ValueError, match="3 entries for 2"):
        m.generate(input_ids=ids, tokenizer=Tok(), generation_config=[g, g, g], seeded_tokens=True)
    with pytest.raises(ValueError, match="token_seed"):
        m.generate(input_ids=ids, tokenizer=Tok(), generation_config=g, token_seed=4)
    with pytest.raises(ValueError, match="device_sampling=False"):
        m.generate(input_ids=ids, tokenizer=Tok(), generation_config=g, seeded_tokens=True, device_sampling=False)
    with pytest.raises(ValueError, match="3 seeds for 2"):
        m.generate(input_ids=ids, tokenizer=Tok(), generation_config=g, seeded_tokens=True, token_seed=[1, 2, 3])
    with pytest.raises(ValueError, match="top_p"):
        m.generate(input_ids=ids, tokenizer=Tok(), generation_config=[g, dict(g, top_p=2.0)], seeded_tokens=True)
    m.seeded_tokens = True                                                                     # the constructor keyword
    with pytest.raises(ValueError, match="device_sampling=False"):
        m.generate(input_ids=ids, tokenizer=Tok(), generation_config=g, device_sampling=False)
    # what generate() hands on: None when no dialogue samples (nothing changes, nothing is drawn), else one row per dialogue
    assert m._token_sampling_args({"do_sample": False}, {}, 2) is None
    assert m._token_sampling_args([{"do_sample": False}, g], {}, 2) == [batchloop.GREEDY_ROW, (0.9, 0, 1.0)]
    assert m._token_sampling_args(g, {"seeded_tokens": False}, 2) is None
    # sessions
    plain = Session(_Fake(), 2, _SPECIAL, _PAD, 4096, _LATENT, max_context=256)
    for kw in (dict(sampler=(1.0, 0, 1.0)), dict(token_seed=5)):
        with pytest.raises(ValueError, match="seeded_tokens"):
            plain.submit(SessionRequest(prompt=torch.arange(5), **kw))
    with pytest.raises(ValueError, match="sample_fn"):
        Session(_Fake(), 2, _SPECIAL, _PAD, 4096, _LATENT, max_context=256, sample_fn=lambda l, i: i[0], seeded_tokens=True)
    with pytest.raises(ValueError, match="device_sampling=False"):
        VibeVoiceSession(m, Tok(), 2, 256, g, True, False, seeded_tokens=True)
    sess = object.__new__(VibeVoiceSession)
    sess.model, sess.seeded_tokens, sess._s = m, False, plain
    with pytest.raises(ValueError, match="seeded_tokens"):
        sess.submit(input_ids=torch.zeros(6, dtype=torch.long), generation_config=g)
    with pytest.raises(ValueError, match="seeded_tokens"):
        sess.submit(input_ids=torch.zeros(6, dtype=torch.long), token_seed=3)
