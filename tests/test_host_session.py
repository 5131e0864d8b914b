"""batchloop.Session - the serving loop that refills finished row-batch slots - under a recording fake driver, on a machine without a GPU:
every dialogue of a session receives the driver calls batchloop.run makes for it alone, admission is FIFO into the lowest free slot, every
request's streamer gets its own chunks and one end(), and the refusals of Session / open_session / generate()."""
import random

import pytest
import torch

from vibevoice_rocm_amd import batchloop
from vibevoice_rocm_amd.batchloop import Session, SessionRequest

_ST, _E, _D, _EOS, _PAD = 150, 151, 152, 153, 7
_SPECIAL = dict(speech_start=_ST, speech_end=_E, speech_diffusion=_D, eos=_EOS, bos=None)
_LATENT = 4


class _Fake:
    """Recording stand-in for the drivers behind batchloop.run and batchloop.Session: returns the forced tokens, speculates every eligible
    dialogue and logs every call as (request, name, details) - the request being the one that occupies the slot at the time (`who`), so a log
    filtered by request reads the same whichever slot served it.  Chunks are small CPU tensors of value 1000 * request + frame."""

    def __init__(self, sde=False, n_steps=3, alone=None):
        self.sde, self.n_steps = sde, n_steps
        self.log, self.who, self.frames, self.ring = [], {}, {}, {}
        self.order, self.history, self.busy = [], {}, set()       # requests in admission order; slot -> requests it served; occupied slots
        if alone is not None:
            self.who, self.frames = {0: alone}, {0: 0}

    def _rec(self, b, name, *detail):
        self.log.append((self.who.get(b), name) + detail)

    @staticmethod
    def _row(row):
        n_row, s_row = row
        if isinstance(n_row, int):
            return ("frame", n_row, s_row)
        return (float(n_row[0]), None if s_row is None else float(s_row[0, 0]))

    # ---- batchloop.run only
    def begin(self, prompts, voices, max_steps, valid):
        assert valid == [_ST, _E, _D, _EOS] and len(prompts) == 1

    def set_noise_seeds(self, seeds):
        self.seeds = list(seeds)

    # ---- batchloop.Session only
    def admit(self, b, req):
        assert b not in self.busy, f"slot {b} admitted into while its occupant is unfinished"
        assert b == min(set(range(self.slots)) - self.busy), "not the lowest free slot"
        self.busy.add(b)
        self.who[b], self.frames[b] = req.tag, 0
        self.order.append(req.tag)
        self.history.setdefault(b, []).append(req.tag)
        self.admitted_with = getattr(self, "admitted_with", []) + [(req.tag, sorted(self.busy - {b}))]

    # ---- both
    def first_tokens(self, live, forced, sample_fn, q=None):
        for b in live:
            self._rec(b, "first", forced[b])
        return {b: forced[b] for b in live}

    def decode(self, live, forced, eligible, sample_fn, deliver, q=None):
        assert set(eligible) <= set(live) == set(forced)
        for b in live:
            self._rec(b, "decode", forced[b], self._row(eligible[b]) if b in eligible else None)
        deliver()
        return {b: forced[b] for b in live}, set(eligible)

    def replace_negative(self, b, src, dst):
        self._rec(b, "replace")

    def rollback(self, b):
        self._rec(b, "rollback")

    def reset_speech(self, b):
        self._rec(b, "reset_speech")

    def embed(self, b):
        self._rec(b, "embed")

    def finished(self, b):
        self._rec(b, "finished")

    def speech(self, rows):
        for b, row in rows.items():
            self._rec(b, "speech", self._row(row))

    def chunk(self, b):
        self._rec(b, "chunk")
        self.frames[b] += 1
        return torch.full((2,), 1000.0 * self.who[b] + self.frames[b] - 1)

    def stage_chunk(self, b):
        self._rec(b, "stage")
        self.ring[(b, self.frames[b] - 1)] = torch.full((2,), 1000.0 * self.who[b] + self.frames[b] - 1)
        return self.frames[b] - 1

    def take_chunk(self, b, slot):
        self._rec(b, "take", slot)
        return self.ring.pop((b, slot))

    def synchronize(self, b=None):
        if b is None and 0 in self.who and not self.busy and not self.order:      # run's epilogue: the one dialogue of the call
            self._rec(0, "sync")
        elif b is not None:
            self._rec(b, "sync")
            self.busy.discard(b)


class _Spy:
    """a batch-of-one streamer that records what it is handed"""

    def __init__(self):
        self.puts, self.ends, self.finished_flags = [], 0, [False]

    def put(self, audio_chunks, sample_indices):
        assert audio_chunks.shape[:2] == (1, 1) and [int(i) for i in sample_indices] == [0]
        assert not self.ends, "a chunk after end()"
        self.puts.append(float(audio_chunks[0, 0, 0]))

    def end(self, sample_indices=None):
        self.ends += 1


def _request(tag, L0, sch, dn, sde, n_steps, max_length_times=50, **kw):
    """request `tag`: prompt of L0 tokens, forced schedule, and - host noise - injected rows whose first element names (request, frame)"""
    req = SessionRequest(prompt=torch.arange(10 + tag, 10 + tag + L0), forced_tokens=list(sch), max_length_times=max_length_times,
                         cfg_scale=1.0 + 0.1 * (tag % 5), **kw)
    if dn:
        req.noise_seed = 7000 + tag
    else:
        F = len(sch) + 1
        req.noise = torch.full((F, _LATENT), 0.0) + (100.0 * tag + torch.arange(F))[:, None]
        if sde:
            req.sde_noise = torch.full((F, n_steps, _LATENT), 0.0) + (100.0 * tag + torch.arange(F))[:, None, None] + 0.5
    req.tag = tag
    return req


def _alone(req, dn, sde, n_steps):
    """batchloop.run on the one dialogue (B = 1) under the same fake: (its log, the output)"""
    drv = _Fake(sde, n_steps, alone=req.tag)
    call = batchloop.BatchCall(special=_SPECIAL, pad_id=_PAD, max_pos=4096, latent=_LATENT, forced_tokens=list(req.forced_tokens),
                               max_new_tokens=req.max_new_tokens, max_length_times=req.max_length_times,
                               noise=req.noise, sde_noise=req.sde_noise, noise_seeds=[req.noise_seed] if dn else None)
    ids = req.prompt[None]
    out = batchloop.run(drv, ids, torch.ones_like(ids), None, None, call)
    return [e[1:] for e in drv.log if e[0] == req.tag], out


def _session(drv, slots, dn, **kw):
    drv.slots = slots
    return Session(drv, slots, _SPECIAL, _PAD, 4096, _LATENT, max_context=kw.pop("max_context", 1024), device_noise=dn, **kw)


def _schedule(rng):
    """turn switches (speech_end / speech_start), runs of frames; ends on EOS - early, late - or not at all (the step limit stops it)"""
    n = rng.randint(1, 14)
    sch = [rng.choice([_D, _D, _D, _D, _E, _ST]) for _ in range(n)]
    return sch + ([_EOS] if rng.random() < 0.75 else [_D] * 40)


def test_session_equals_alone():
    """Random scripts: 2..8 slots, 6..20 requests arriving at random steps with random schedules.  Every dialogue receives - admit aside - the
    ordered driver calls batchloop.run makes for it alone (rollback, reset_speech and embed among them), and ends with the same sequence, frame
    count and reach_max.  Over the script set mid-flight admission, slot reuse, queue wait and rollback each occur often."""
    rng = random.Random(20)
    seen = dict(midflight=0, reuse=0, waited=0, rollback=0, reset_speech=0, embed=0, step_limit=0)
    for it in range(240):
        slots, n_req = rng.randint(2, 8), rng.randint(6, 20)
        dn, sde, n_steps = bool(it % 2), bool((it // 2) % 2), 3
        drv = _Fake(sde, n_steps)
        sess = _session(drv, slots, dn)
        reqs, arrive = [], []
        for tag in range(n_req):
            L0 = rng.randint(3, 9)
            sch = _schedule(rng)
            reqs.append(_request(tag, L0, sch, dn, sde, n_steps, max_length_times=rng.choice([2, 3, 50] if sch[-1] == _EOS else [2, 3])))
            arrive.append(rng.randint(0, 12))
        arrive.sort()
        handles, t, waited = {}, 0, set()
        while True:
            for tag in range(n_req):
                if arrive[tag] == t:
                    handles[tag] = sess.submit(reqs[tag])
            going = sess.step()
            waited |= {tag for tag, h in handles.items() if h.slot is None and not h.done}
            t += 1
            if not going and t > arrive[-1]:
                break
            assert t < 2000
        sess.close()
        assert drv.order == list(range(n_req))                                   # FIFO
        for tag, req in enumerate(reqs):
            want_log, want = _alone(req, dn, sde, n_steps)
            got_log = [e[1:] for e in drv.log if e[0] == tag]
            assert got_log == want_log, (it, tag, req.forced_tokens, got_log, want_log)
            got = handles[tag].result()
            assert handles[tag].done and got.sequences.tolist() == want.sequences.tolist(), (it, tag)
            assert got.reach_max_step_sample.tolist() == want.reach_max_step_sample.tolist()
            assert (got.speech_outputs[0] is None) == (want.speech_outputs[0] is None)
            if want.speech_outputs[0] is not None:
                assert torch.equal(got.speech_outputs[0], want.speech_outputs[0])
            names = [e[0] for e in got_log]
            for k in ("rollback", "reset_speech", "embed"):
                seen[k] += names.count(k)
            seen["step_limit"] += "finished" not in names
        seen["midflight"] += sum(1 for tag, others in drv.admitted_with if _was_running(drv, tag, others))
        seen["reuse"] += sum(len(v) - 1 for v in drv.history.values())
        seen["waited"] += len(waited)
    assert min(seen.values()) >= 20, seen


def _was_running(drv, tag, others):
    """at the admission of `tag` an occupant of another slot had already taken a decode step: the admission happened mid-flight"""
    first = next(i for i, e in enumerate(drv.log) if e[0] == tag)
    return any(e[0] in others and e[1] == "decode" for e in drv.log[:first])


def test_admission_is_fifo_into_the_lowest_free_slot():
    """Six requests on two slots: the fake refuses an admission into an occupied slot or past a lower free one (asserted in _Fake.admit);
    requests start in the order they were submitted, and the dialogue that ends first hands ITS slot to the next in the queue."""
    drv = _Fake()
    sess = _session(drv, 2, True)
    sch = [[_ST, _D, _D, _D, _D, _E, _EOS], [_ST, _D, _EOS], [_ST, _D, _D, _EOS], [_EOS], [_ST, _D, _E, _EOS], [_ST, _EOS]]
    hs = [sess.submit(_request(tag, 4, s, True, False, 3)) for tag, s in enumerate(sch)]
    assert [h.slot for h in hs] == [None] * 6 and not any(h.done for h in hs)
    assert sess.step() and [h.slot for h in hs] == [0, 1, None, None, None, None]
    sess.run()
    assert drv.order == [0, 1, 2, 3, 4, 5] and all(h.done for h in hs)
    assert [h.slot for h in hs] == [0, 1, 1, 1, 1, 0]       # request 1 ends first: 2 takes slot 1; 3 ends on its first token: 4 takes slot 1 in the same step ...
    assert drv.history == {0: [0, 5], 1: [1, 2, 3, 4]}
    assert not sess.step() and not drv.busy
    for h, s in zip(hs, sch):
        assert h.result().sequences[0, 4:].tolist() == s


def test_streamers_and_cancellation():
    """Each request's streamer gets exactly its own chunks, in order, and one end() - on EOS, on the step limit, on cancel() and on
    stop_check_fn; a cancelled dialogue frees its slot on the next step, a cancelled queued one never starts."""
    drv = _Fake()
    sess = _session(drv, 2, True)
    spies = [_Spy() for _ in range(5)]
    polls = []
    sch = [[_ST] + [_D] * 5 + [_E, _EOS],        # 0: EOS
           [_ST] + [_D] * 30,                    # 1: prompt of 4, max_length_times 2 -> 8 steps: the step limit
           [_ST] + [_D] * 30,                    # 2: cancelled after three steps
           [_ST] + [_D] * 30,                    # 3: stop_check_fn fires at its fifth poll
           [_ST, _D, _EOS]]                      # 4: cancelled while queued
    kw = [dict(), dict(max_length_times=2), dict(), dict(stop_check_fn=lambda: polls.append(0) or len(polls) == 5), dict()]
    hs = [sess.submit(_request(tag, 4, s, True, False, 3, audio_streamer=spies[tag], **kw[tag])) for tag, s in enumerate(sch)]
    hs[4].cancel()
    while not (hs[0].done and hs[1].done):
        sess.step()
    assert [h.slot for h in hs[:2]] == [0, 1] and hs[4].done and hs[4].slot is None and spies[4].ends == 1 and not spies[4].puts
    assert hs[4].result().sequences[0].tolist() == list(range(14, 18)) and hs[4].result().speech_outputs == [None]
    assert spies[0].puts == [0.0 + f for f in range(5)] and spies[0].ends == 1
    assert spies[1].puts == [1000.0 + f for f in range(7)] and spies[1].ends == 1 and hs[1].result().sequences.shape[1] == 4 + 8
    assert not hs[1].result().reach_max_step_sample.any()         # a batch of one runs out of steps (batchloop.run: the flag stays False)
    for _ in range(3):
        sess.step()
    where = hs[2].slot
    assert where is not None and not hs[2].done
    hs[2].cancel()
    n = len(spies[2].puts)
    busy = set(drv.busy)
    sess.step()
    assert hs[2].done and spies[2].ends == 1 and where not in drv.busy and where in busy
    assert len(spies[2].puts) >= n and spies[2].puts == [2000.0 + f for f in range(len(spies[2].puts))]
    assert hs[2].result().speech_outputs[0][0, ::2].tolist() == spies[2].puts          # every frame it generated was delivered before end()
    sess.run()
    assert hs[3].done and spies[3].ends == 1 and len(polls) == 5
    assert hs[3].result().sequences[0, 4:].tolist() == sch[3][:4] and spies[3].puts == [3000.0, 3001.0, 3002.0]
    assert [s.ends for s in spies] == [1] * 5 and not drv.ring
    sess.close()
    assert sess.closed and not sess.step()


def test_refusals():
    """slots out of range; a context that does not fit at submit; noise= in a device-noise session and a seed in a host-noise one; a second
    open session; generate() while a session is open; a cfg_scale list of the wrong length in generate().  The model-level refusals come
    before anything touches the device, so a bare instance shows them."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as Model
    for slots in (0, 1, 17, 2.5):
        with pytest.raises(ValueError):
            _session(_Fake(), slots, True)
    with pytest.raises(ValueError):
        _session(_Fake(), 4, True, max_context=None)
    sess = _session(_Fake(), 2, True, max_context=64)
    sess.submit(_request(0, 10, [_EOS], True, False, 3, max_length_times=2))                 # 10 + 20 + 8 <= 64
    with pytest.raises(ValueError, match="max_context"):
        sess.submit(_request(1, 20, [_EOS], True, False, 3, max_length_times=2))             # 20 + 40 + 8 > 64: refused, not clipped
    sess.submit(_request(2, 20, [_EOS], True, False, 3, max_new_tokens=30))                  # 20 + 30 + 8 <= 64
    with pytest.raises(ValueError, match="device_noise"):
        sess.submit(_request(3, 4, [_EOS], False, False, 3))                                 # carries noise=
    with pytest.raises(ValueError, match="device_noise"):
        _session(_Fake(), 2, False).submit(_request(4, 4, [_EOS], True, False, 3))           # carries noise_seed=
    assert len(sess.queue) == 2
    torch.manual_seed(5)
    h = sess.submit(SessionRequest(prompt=torch.arange(4), forced_tokens=[_EOS]))            # no seed given: drawn from the CPU generator
    torch.manual_seed(5)
    assert h.request.noise_seed == int(torch.randint(0, 2 ** 62, (1,)))
    with pytest.raises(RuntimeError):
        h.result()
    sess.close()
    with pytest.raises(RuntimeError):
        sess.submit(_request(5, 4, [_EOS], True, False, 3))

    class Tok:
        speech_start_id, speech_end_id, speech_diffusion_id, eos_token_id = _ST, _E, _D, _EOS

    m = object.__new__(Model)
    m._session, m.dtype, m.weight_quant, m.kv_cache_dtype, m._use_graphs = None, torch.bfloat16, None, None, True
    for bad in (1, 17):
        with pytest.raises(ValueError, match="slots"):
            m.open_session(tokenizer=Tok(), slots=bad, max_context=256)
    with pytest.raises(ValueError, match="max_context"):
        m.open_session(tokenizer=Tok(), slots=4)
    for attr, val in (("dtype", torch.float32), ("weight_quant", "nf4"), ("kv_cache_dtype", "fp8"), ("_use_graphs", False)):
        old = getattr(m, attr)
        setattr(m, attr, val)
        with pytest.raises(ValueError, match="row-batched"):
            m.open_session(tokenizer=Tok(), slots=4, max_context=256)
        setattr(m, attr, old)
    m._session = object()
    with pytest.raises(RuntimeError, match="session"):
        m.open_session(tokenizer=Tok(), slots=4, max_context=256)
    with pytest.raises(RuntimeError, match="session"):
        m.generate(input_ids=torch.zeros(1, 4, dtype=torch.long), tokenizer=Tok())
    m._session = None
    with pytest.raises(ValueError, match="cfg_scale"):
        m.generate(input_ids=torch.zeros(2, 4, dtype=torch.long), tokenizer=Tok(), cfg_scale=[1.3, 2.0, 3.0])
    with pytest.raises(ValueError, match="cfg_scale"):
        m.generate(input_ids=torch.zeros(4, dtype=torch.long), tokenizer=Tok(), cfg_scale=[1.3, 2.0])


def test_abi_entry():
    import ctypes as C
    from vibevoice_rocm_amd import _lib
    res, args = _lib.PROTOTYPES["vv_head_sample_batch_cfg"]
    vp, i64 = C.c_void_p, C.c_int64
    assert res is C.c_int and args == [C.POINTER(_lib.Head), vp, i64, vp, i64, vp, C.POINTER(_lib.DpmCoef), C.c_int, vp, vp, i64, C.c_int, vp, vp, i64, vp]
    assert hasattr(_lib.load(), "vv_head_sample_batch_cfg")
