"""The batched generate() loop (reference: modeling_vibevoice_inference.py:430-673 with batch_size > 1), written once, and the small host
helpers the batch-of-one path shares with it (valid ids, limits, output packing).

`run` is host bookkeeping only - limits, the token state machine, the batch coupling, which frames may be speculated, the reference-order
noise draws, chunk collection and streaming.  It makes no torch.cuda call and knows no Engine, RowBatch or stream: all of that sits behind a
driver (modeling._LaneDriver: one Engine lane per dialogue; modeling._RowDriver: RowBatch groups of 2..4 dialogues, 2..8 at row_batch_width=8), so the loop runs under
a recording fake on a machine without a GPU (tests/test_host_cpu.py).  A driver has the attributes `sde`, `n_steps` and the methods

  begin(prompts, voices, max_steps, valid)   fresh sequences; prompt embeddings with the voice rows `(mask, rows)` scattered in
  first_tokens(live, forced, sample_fn)      step 0: prefill of every live dialogue, first token, negative prompt committed where it diffuses
  decode(live, forced, eligible, sample_fn, deliver)
                                             one LLM step: {dialogue: token} and the set of dialogues whose frame it speculated (a subset of
                                             `eligible` = {dialogue: (noise row, SDE rows)}); calls deliver() once, before it first waits
  replace_negative(b, src, dst)              negative KV slot src -> dst            rollback(b)      undo a mis-speculated frame
  reset_speech(b)                            zero the conv states                   embed(b)         next input = embedding of its token
  finished(b)                                the dialogue takes no more steps
  speech(rows)                               the frame of every dialogue in {dialogue: (noise row, SDE rows)}; all launches enqueued on return
  chunk(b) / stage_chunk(b) / take_chunk(b, slot)     the frame's samples (device), its copy to the host ring, the host samples
  synchronize()

do_sample on the device (BatchCall.sampler): the driver is told the warpers once (`set_sampler(temperature, top_k, top_p)`), sample_fn is None and
first_tokens / decode get `q=` {dialogue: its exponential draws [nv]} for the live dialogues without a forced token; the token comes back
like a greedy one.

Seeded token draws (BatchCall.token_sampling): the driver is told every dialogue's own warpers and 64-bit token seed once
(`set_token_sampling(samplers, seeds)`, after begin; a greedy dialogue's row is (0, 0, 1)) and draws each token on the device from (the
dialogue's seed, the position, its logits): sample_fn is None, no `q` is passed and the loop makes no draw of its own.

Diffusion noise on the device (BatchCall.noise_seeds): the driver is told every dialogue's seed once (`set_noise_seeds(seeds)`, after begin) and
draws a frame's noise itself from (seed, frame index); `eligible` and the rows of `speech` then carry `(frame index, None)` in place of the
noise rows, every dialogue in its steady state may be speculated, and the loop makes no draw of its own.

`Session` (below `run`) is the same loop for serving: slots that are refilled between two steps, every dialogue with batch-of-one semantics
(modeling._SessionDriver; under a recording fake in tests/test_host_session.py)."""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch


@dataclass
class VibeVoiceGenerationOutput:
    sequences: torch.LongTensor = None
    speech_outputs: Optional[List[Optional[torch.Tensor]]] = None
    reach_max_step_sample: Optional[torch.BoolTensor] = None


@dataclass
class BatchCall:
    """What one generate() call fixes for its batched loop.  `forced_tokens` / `noise` / `sde_noise` may be given per sample (list / leading
    batch dimension) or once for all."""
    special: dict                         # speech_start / speech_end / speech_diffusion / eos [/ bos] ids
    pad_id: int
    max_pos: int
    latent: int
    max_new_tokens: Optional[int] = None
    max_length_times: float = 2
    forced_tokens: Optional[list] = None
    noise: Optional[torch.Tensor] = None
    sde_noise: Optional[torch.Tensor] = None
    audio_streamer: object = None
    stop_check_fn: Optional[Callable[[], bool]] = None
    verbose: bool = False
    sample_fn: Optional[Callable] = None
    sampler: Optional[tuple] = None       # do_sample on the device: the warpers (temperature, top_k, top_p); sample_fn is None then
    token_sampling: Optional[tuple] = None    # seeded token draws: ([(temperature, top_k, top_p)] * B, [64-bit seed] * B); sampler / sample_fn are None then
    noise_seeds: Optional[List[int]] = None   # diffusion noise on the device: one 64-bit seed per dialogue; noise / sde_noise are None then
    speculate: bool = True                # frames may be launched before their token is known (never with sample_fn)
    return_speech: bool = True
    in_dev: object = "cpu"


def valid_token_ids(special: dict) -> List[int]:
    """the ids generation is constrained to (modeling_vibevoice_inference.py:53-66)"""
    return [special["speech_start"], special["speech_end"], special["speech_diffusion"], special["eos"]] + \
        ([special["bos"]] if special.get("bos") is not None else [])


def sampler_params(gen_cfg: dict) -> tuple:
    """(temperature, top_k, top_p) as modeling._make_sampler reads them from a generation_config dict"""
    return (float(gen_cfg.get("temperature", 1.0) or 1.0), int(gen_cfg.get("top_k", 0) or 0), float(gen_cfg.get("top_p", 1.0) or 1.0))


GREEDY_ROW = (0.0, 0, 1.0)      # the sampler row of a dialogue that takes the argmax (seeded token draws)


def sampler_row(gen_cfg: Optional[dict]) -> tuple:
    """The vv_sampler row of one dialogue's generation_config under seeded token draws: GREEDY_ROW without do_sample, else its warpers.
    ValueError for warpers outside the kernels' contract (temperature > 0 when sampling, 0 < top_p <= 1)."""
    g = dict(gen_cfg or {})
    if not g.get("do_sample", False):
        return GREEDY_ROW
    t, k, p = sampler_params(g)
    if not (0.0 < t < float("inf")) or not (0.0 < p <= 1.0):
        raise ValueError(f"generation_config: temperature={t!r} (> 0) / top_p={p!r} (0 < top_p <= 1)")
    return (t, max(k, 0), p)


def draw_q(nv: int) -> torch.Tensor:
    """The draws torch.multinomial(p, 1) makes on the CPU for nv probabilities - q = empty_like(p).exponential_(1), token = argmax(p / q) - from
    the default generator, which is left where multinomial leaves it.  They do not depend on p: the device finishes the choice (vv_sampler)."""
    return torch.empty(nv, dtype=torch.float32).exponential_(1)


def limits(max_pos: int, prompt_len: int, max_new_tokens: Optional[int], max_length_times: float):
    """(max_length, max_steps) of a call whose (padded) prompt has prompt_len tokens"""
    max_length = max_pos if max_new_tokens is None else prompt_len + int(max_new_tokens)            # :370-371
    return max_length, min(max_length - prompt_len, int(max_length_times * prompt_len))            # :420


def pack_output(rows: List[torch.Tensor], audios, reach: List[bool], pad_id: int, in_dev, return_speech: bool) -> VibeVoiceGenerationOutput:
    """rows: every sample's ids (left padding included), right-padded here to the longest"""
    seq_t = torch.full((len(rows), max(r.shape[0] for r in rows)), int(pad_id), dtype=torch.long)
    for b, r in enumerate(rows):
        seq_t[b, : r.shape[0]] = r
    return VibeVoiceGenerationOutput(sequences=seq_t.to(in_dev), speech_outputs=audios if return_speech else None,
                                     reach_max_step_sample=torch.tensor(reach, dtype=torch.bool))


class _BatchCoupling:
    """Where the reference's BATCHED loop does not treat a sample as if it ran alone; the host knows every step's tokens, so it can say.
    (1) Negative branch (modeling_vibevoice_inference.py:575-622): one negative forward for all samples whenever any diffuses, then the
        non-diffusing ones are shifted out from their correct_cnt.  The mask guard tests seq_len - 1, the KV guard k_cache.shape[2] - 1,
        one row shorter: with correct_cnt == kv_len - 2 the mask moves one slot right and the rows do not, so the row just computed for
        the sample stays visible in place of its last visible one.  `replace` lists those dialogues: their negative row of this step
        (computed by every decode step anyway, at slot lens[1]) is copied over slot lens[1] - 1 and lens[1] stays.
    (2) Streaming tokenizer cache (modular_vibevoice_tokenizer.py:198-207): get() returns None - a fresh conv state for the whole call -
        when one sample of the diffusing subset has no state yet.  `restart` lists the dialogues whose conv states are zeroed before
        this frame's tail because they diffuse next to a first-time diffuser.
    Neither applies to a batch of one.  Restated symbolically, literal to the reference, by the CPU restatement the tests use (batch_negative_replacements,
    batch_conv_restarts) and pinned by tests/golden/loop_trace_batch_*."""

    def __init__(self, B: int, tok_start: int, tok_diff: int):
        self.ST, self.SD = tok_start, tok_diff
        self.n_fwd = 0                 # negative forwards so far (the batch-wide negative cache length)
        self.cnt = [0] * B             # correct_cnt
        self.vis = [0] * B             # visible negative rows of each dialogue (= its lens[1])
        self.seen = [False] * B        # has a streaming tokenizer state

    def step(self, toks: Dict[int, int], going: List[int]):
        """toks: this step's token of every dialogue live at its start; going: those still unfinished after it (no EOS, no max length).
        Returns (replace, restart)."""
        diff = [b for b in going if toks[b] == self.SD]
        for b in going:
            if toks[b] == self.ST:
                self.vis[b] = 0
        replace, restart = [], []
        if diff:
            self.n_fwd += 1
            for b in going:
                if toks[b] != self.SD:
                    if self.cnt[b] == self.n_fwd - 2 and self.vis[b] >= 1:
                        replace.append(b)
                    self.cnt[b] += 1
            if not all(self.seen[b] for b in diff):
                restart = [b for b in diff if self.seen[b]]
            for b in diff:
                self.seen[b] = True
                self.vis[b] += 1
        return replace, restart


def run(driver, input_ids: torch.Tensor, attention_mask: torch.Tensor, speech_input_mask, conn_all, call: BatchCall) -> VibeVoiceGenerationOutput:
    """One host loop drives B dialogues in lock step, as the reference's batched generate() does: every live sample takes its LLM step (all
    of them enqueued before any token is awaited), tokens are handled per sample (:517-563), the samples that emitted speech_diffusion are
    sampled / decoded / re-embedded (:571-670) and their chunks reach the AudioStreamer together, once per step (:644-653).  The random
    draws follow the reference's order (randn(2 n, latent) per step for the n diffusing samples, rows [:n] used, :699; SDE solver: n_steps
    more of the same, dpm_solver.py:993-998) - only for the dialogues that diffuse, were not speculated and have no injected row, in ascending order."""
    B, Lp = input_ids.shape
    special, streamer, sample_fn = call.special, call.audio_streamer, call.sample_fn
    ST, SE, SD, EOS = special["speech_start"], special["speech_end"], special["speech_diffusion"], special["eos"]
    keep = attention_mask.bool()
    L0 = keep.sum(-1).tolist()
    max_length, max_steps = limits(call.max_pos, Lp, call.max_new_tokens, call.max_length_times)     # padded length, as the reference
    max_step_per_sample = [min(max_length - l, int(call.max_length_times * l)) for l in L0]         # :421
    forced_tokens, noise, sde_noise = call.forced_tokens, call.noise, call.sde_noise
    per_list = forced_tokens is not None and len(forced_tokens) > 0 and isinstance(forced_tokens[0], (list, tuple))
    ftok = [(forced_tokens[b] if per_list else forced_tokens) for b in range(B)]
    nz = [(noise[b] if (noise is not None and noise.dim() == 3) else noise) for b in range(B)]
    snz = [(sde_noise[b] if (sde_noise is not None and sde_noise.dim() == 4) else sde_noise) for b in range(B)]
    prompts = [input_ids[b][keep[b]] for b in range(B)]
    voices, off = [None] * B, 0
    if speech_input_mask is not None and conn_all is not None:
        for b in range(B):
            sp_b = speech_input_mask[b][keep[b]].bool()
            n_b = int(sp_b.sum())
            if n_b:
                voices[b] = (sp_b, conn_all[off: off + n_b])
                off += n_b
    driver.begin(prompts, voices, max_steps, valid_token_ids(special))
    sde, n_steps = driver.sde, driver.n_steps
    seq = [p.tolist() for p in prompts]
    chunks = [[] for _ in range(B)]
    frame = [0] * B
    finished = [False] * B
    reach = [False] * B
    prev_tok = [None] * B
    pending = []                      # (sample, ring slot) of chunks not yet handed to the streamer
    ours = [False] * max(B, getattr(streamer, "batch_size", B) if streamer is not None else B)   # streams ended by this loop
    speculate = call.speculate and sample_fn is None
    nv = len(set(valid_token_ids(special)))
    if call.sampler is not None:
        if sample_fn is not None:
            raise ValueError("BatchCall: sampler (device) and sample_fn (host) exclude each other")
        driver.set_sampler(*call.sampler)
    if call.token_sampling is not None:
        if sample_fn is not None or call.sampler is not None:
            raise ValueError("BatchCall: token_sampling (seeded draws on the device) excludes sampler and sample_fn")
        rows_, seeds_ = call.token_sampling
        if len(rows_) != B or len(seeds_) != B:
            raise ValueError(f"BatchCall: token_sampling has {len(rows_)} sampler rows and {len(seeds_)} seeds for {B} dialogues")
        driver.set_token_sampling([tuple(r) for r in rows_], [int(s_) for s_ in seeds_])
    dn = call.noise_seeds is not None
    if dn:
        if noise is not None or sde_noise is not None:
            raise ValueError("BatchCall: noise_seeds (drawn on the device) and injected noise / sde_noise exclude each other")
        if len(call.noise_seeds) != B:
            raise ValueError(f"BatchCall: noise_seeds has {len(call.noise_seeds)} entries for {B} dialogues")
        driver.set_noise_seeds([int(s_) for s_ in call.noise_seeds])
    coupling = _BatchCoupling(B, ST, SD)

    def deliver():
        if streamer is not None and pending:
            streamer.put(torch.stack([driver.take_chunk(b, k)[None] for b, k in pending]), torch.tensor([b for b, _ in pending]))   # one put per step, all samples (:644-653)
        pending.clear()

    def finish(b):
        finished[b] = True
        driver.finished(b)
        if streamer is not None:
            deliver()
            ours[b] = True
            streamer.end(torch.tensor([b]))

    for step in range(max_steps):
        if call.stop_check_fn is not None and call.stop_check_fn():                                 # :432-438
            if call.verbose:
                print(f"Generation stopped externally at step {step + 1}")
            deliver()
            if streamer is not None:
                streamer.end()
            break
        if streamer is not None and hasattr(streamer, "finished_flags") and any(f and not ours[i] for i, f in enumerate(streamer.finished_flags)):
            break           # :441-445 "stopped externally".  Deviation, on purpose: the reference tests any(finished_flags), which its own
                            # end(new_eos_indices) at :526 also sets - a batch with a streamer then stops at the FIRST sample's EOS; here
                            # only streams ended by someone else stop the batch, streams this loop ended itself (EOS / max length) do not
        if all(finished):
            break
        if Lp + step >= max_length:                                                                 # :452-457
            for b in range(B):
                reach[b] = reach[b] or not finished[b]
            break
        live = [b for b in range(B) if not finished[b]]
        forced = {b: (ftok[b][step] if (ftok[b] is not None and step < len(ftok[b])) else None) for b in live}
        # device-side do_sample: one exponential_ per live dialogue without a forced token, in ascending order - where the host sampler's
        # multinomial draws them.  Batches speculate with injected noise only, so no other draw can come between these and the token
        kw = {} if call.sampler is None else dict(q={b: draw_q(nv) for b in live if forced[b] is None})
        if step == 0:
            toks, speculated = driver.first_tokens(live, forced, sample_fn, **kw), set()
        else:
            # a dialogue in its steady state may get its diffusion tail enqueued speculatively behind its LLM step when its noise is injected
            # (drawn noise depends on how many samples diffuse in this step, which is only known once the tokens are)
            if dn:
                # noise drawn on the device: a frame's noise is a function of its index, whoever else diffuses and whether or not it was speculated
                eligible = {b: (frame[b], None) for b in live if speculate and prev_tok[b] == SD}
            else:
                eligible = {b: (nz[b][frame[b]], snz[b][frame[b]] if sde else None) for b in live
                            if speculate and prev_tok[b] == SD and nz[b] is not None and frame[b] < len(nz[b]) and
                            (not sde or (snz[b] is not None and frame[b] < len(snz[b])))}
            toks, speculated = driver.decode(live, forced, eligible, sample_fn, deliver, **kw)
        going = [b for b in live if toks[b] != EOS and step < max_step_per_sample[b]]
        replace, restart = coupling.step(toks, going)
        for b in replace:
            driver.replace_negative(b, coupling.vis[b], coupling.vis[b] - 1)
        diffusing = []
        for b in live:
            tok = toks[b]
            if b in speculated and (tok != SD or b in restart):
                driver.rollback(b)
                speculated.discard(b)
            prev_tok[b] = tok
            seq[b].append(tok)
            if tok == EOS:                                                                          # :517-526
                if call.verbose:
                    print(f"Samples [{b}] reached EOS token at step {step + 1}.", flush=True)
                finish(b)
                continue
            if step >= max_step_per_sample[b]:                                                      # :528-537
                reach[b] = True
                finish(b)
                continue
            if tok == SE:                                                                           # :540-544
                driver.reset_speech(b)
            if tok == SD:
                diffusing.append(b)
                if b in restart:
                    driver.reset_speech(b)
            else:
                driver.embed(b)                                                                     # :567
        need = [] if dn else [b for b in diffusing if b not in speculated and (nz[b] is None or frame[b] >= len(nz[b]))]
        if need:
            n = len(need)
            drawn = torch.randn(2 * n, call.latent)[:n]
            sdrawn = torch.stack([torch.randn(2 * n, call.latent)[:n] for _ in range(n_steps)], dim=1) if sde else None
        rows = {}
        for b in diffusing:                                                                         # :571-670
            if b in need:
                i = need.index(b)
                rows[b] = (drawn[i], sdrawn[i] if sde else None)
            elif b not in speculated:
                rows[b] = (frame[b], None) if dn else (nz[b][frame[b]], snz[b][frame[b]] if sde else None)
        driver.speech(rows)
        for b in diffusing:
            chunks[b].append(driver.chunk(b))
            if streamer is not None:
                pending.append((b, driver.stage_chunk(b)))
            frame[b] += 1
    deliver()
    driver.synchronize()
    if streamer is not None:
        streamer.end()
    rows = [torch.cat([input_ids[b][~keep[b]], torch.tensor(seq[b], dtype=torch.long)]) for b in range(B)]
    audios = [(torch.cat(c)[None] if c else None) for c in chunks]
    return pack_output(rows, audios, reach, call.pad_id, call.in_dev, call.return_speech)


# ---------------------------------------------------------------------------------------------------------------------
# serving sessions: the row batches' slots refilled between two steps
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class SessionRequest:
    """What submit() fixes for one dialogue of a session: its unpadded prompt (`head`: the left padding the caller's row carried, put back in front
    of the returned sequence), its voice rows `(mask, rows)` or voice prefix, its guidance scale, limits, schedule, noise and streamer."""
    prompt: torch.Tensor
    head: Optional[torch.Tensor] = None
    voice: Optional[tuple] = None
    prefix: object = None
    cfg_scale: float = 1.0
    max_new_tokens: Optional[int] = None
    max_length_times: float = 2
    forced_tokens: Optional[list] = None
    noise: Optional[torch.Tensor] = None          # [F, latent] (host-noise sessions)
    sde_noise: Optional[torch.Tensor] = None      # [F, n_steps, latent]
    noise_seed: Optional[int] = None              # device-noise sessions; None: drawn from the CPU generator at submit
    sampler: Optional[tuple] = None               # seeded-token sessions: this request's (temperature, top_k, top_p), GREEDY_ROW = greedy; None: the session's
    token_seed: Optional[int] = None              # seeded-token sessions; None: drawn from the CPU generator at submit, after the noise seed
    audio_streamer: object = None                 # a batch-of-one streamer of this request's own
    stop_check_fn: Optional[Callable[[], bool]] = None
    in_dev: object = "cpu"


class SessionHandle:
    """One submitted dialogue: `done`, the `slot` it runs / ran in (None while queued), `cancel()` - it leaves at the session's next step - and
    `result()`, the VibeVoiceGenerationOutput of a batch of one."""

    def __init__(self, req: SessionRequest):
        self.request, self.done, self.slot, self.cancelled, self._out = req, False, None, False, None

    def cancel(self):
        self.cancelled = True

    def result(self) -> VibeVoiceGenerationOutput:
        if not self.done:
            raise RuntimeError("SessionHandle.result(): the dialogue has not finished (Session.step() / run())")
        return self._out


class _Dialogue:
    def __init__(self, handle: SessionHandle, max_length: int, max_steps: int):
        r = handle.request
        self.handle, self.req = handle, r
        self.L0, self.max_length, self.max_steps = int(r.prompt.shape[0]), max_length, max_steps
        self.seq = r.prompt.tolist()
        self.chunks, self.frame, self.prev_tok, self.step, self.reach = [], 0, None, 0, False


class Session:
    """`run`'s loop turned inside out for serving: a fixed number of slots (the row batches' dialogues) that are refilled between two steps, so a
    finished dialogue costs nothing further and a queued one starts as soon as a slot is free.  Every dialogue is served with BATCH-OF-ONE
    semantics - its limits from its own unpadded prompt, its own step counter from its admission, no _BatchCoupling (both of that class's
    effects only mimic the reference's batched call) - so it receives, in order, the driver calls `run` makes for it alone; speech_end resets,
    turn switches, the negative commit, speculation and rollback are `run`'s.

    The driver is `run`'s (module docstring) without `begin`, opened by the caller, plus
      admit(b, request)          slot b starts afresh for this request: its positions, conv state, guidance scale, noise seed, sampler row / token seed and prompt embeddings
      synchronize(b)             everything enqueued for slot b has completed (its samples may be read)
    and `decode(live, ...)` leaves the slots outside `live` where they are.  One step(): (1) queued requests are admitted in FIFO order while
    a slot is free, lowest free slot first - admit, first_tokens([b]) (the prefill and the first token), that token handled - synchronously;
    (2) one decode for every live dialogue; (3) tokens, speech, chunk delivery.

    Noise is the session's: `device_noise` (default) gives every request its own seed and draws on the device, a frame's noise a function of
    (seed, frame) - the dialogue sounds the same whoever shares the session; noise= / sde_noise= are refused.  Without it noise is injected per
    request or drawn on the host as `run` draws it, and drawn noise then depends on who else diffuses in the step (not reproducible per
    dialogue).  Tokens: greedy, forced per request, or sampled with the session's one sampler (`sample_fn` on the host or `sampler` = the
    device's warpers); the draws of a step are made in ascending slot order.  `seeded_tokens`: every request brings its own warpers
    (`SessionRequest.sampler`, default the session's `sampler`, greedy without one) and token seed, which reach the driver through `admit`; the
    tokens are drawn on the device from (seed, position, logits), first_tokens / decode get neither `q` nor a sample_fn and no draw is made here -
    a dialogue's tokens are the same whoever shares the session."""

    def __init__(self, driver, slots: int, special: dict, pad_id: int, max_pos: int, latent: int, max_context: int, device_noise: bool = True,
                 sample_fn=None, sampler: Optional[tuple] = None, speculate: bool = True, verbose: bool = False, on_close=None,
                 seeded_tokens: bool = False, packed_prefill: bool = False):
        if not isinstance(slots, int) or not 2 <= slots <= 16:
            raise ValueError(f"Session: slots={slots!r} (2..16)")
        if max_context is None or int(max_context) <= 0:
            raise ValueError(f"Session: max_context={max_context!r} (tokens per dialogue, required)")
        if sampler is not None and sample_fn is not None:
            raise ValueError("Session: sampler (device) and sample_fn (host) exclude each other")
        if seeded_tokens and sample_fn is not None:
            raise ValueError("Session: seeded_tokens draws the tokens on the device: it excludes sample_fn (the host sampler)")
        self.seeded_tokens = bool(seeded_tokens)
        self.packed_prefill = bool(packed_prefill)      # _admit: every queued request that finds a slot, then ONE first_tokens call for them all
        self.default_row = (tuple(sampler) if sampler is not None else GREEDY_ROW) if self.seeded_tokens else None
        if self.seeded_tokens:
            sampler = None                # no session-wide warpers on the driver, no q: every request's row travels with its admission
        self.driver, self.slots, self.special, self.pad_id, self.max_pos, self.latent = driver, slots, special, int(pad_id), int(max_pos), int(latent)
        self.max_context, self.device_noise, self.sample_fn, self.sampler, self.verbose = int(max_context), bool(device_noise), sample_fn, sampler, verbose
        self.speculate = bool(speculate) and sample_fn is None
        self.nv = len(set(valid_token_ids(special)))
        self.queue: List[SessionHandle] = []
        self.live: Dict[int, _Dialogue] = {}
        self.pending = []                 # (dialogue, slot, ring slot) of chunks not yet handed to their streamers
        self.admissions = []              # (slot, dialogues live at the time) per admission, in order
        self.admission_ms = []            # and how long the host spent on it (admit + prefill + first token, synchronous)
        self.closed, self._on_close = False, on_close
        if sampler is not None:
            driver.set_sampler(*sampler)

    # ---- requests ---------------------------------------------------------------------------------------------------
    def limits_of(self, prompt_len: int, max_new_tokens, max_length_times):
        return limits(self.max_pos, prompt_len, max_new_tokens, max_length_times)

    def validate(self, req: SessionRequest):
        """submit()'s refusals, without queueing or drawing anything"""
        if self.closed:
            raise RuntimeError("Session.submit(): the session is closed")
        if self.device_noise:
            if req.noise is not None or req.sde_noise is not None:
                raise ValueError("this session draws the diffusion noise on the device (device_noise=True): noise= / sde_noise= cannot be injected")
        elif req.noise_seed is not None:
            raise ValueError("noise_seed= seeds the device-side noise: it needs a session opened with device_noise=True")
        if not self.seeded_tokens and (req.sampler is not None or req.token_seed is not None):
            raise ValueError("generation_config= / token_seed= per request need a session opened with seeded_tokens=True (this session has one sampler)")
        L0 = int(req.prompt.shape[0])
        if L0 < 1:
            raise ValueError("Session.submit(): empty prompt")
        _, max_steps = self.limits_of(L0, req.max_new_tokens, req.max_length_times)
        if L0 + max(max_steps, 1) + 8 > self.max_context:
            raise ValueError(f"Session.submit(): prompt of {L0} tokens + step limit {max_steps} + 8 = {L0 + max(max_steps, 1) + 8} exceeds the session's "
                             f"max_context={self.max_context} (lower max_new_tokens / max_length_times, or open the session with a larger max_context)")

    def submit(self, req: SessionRequest) -> SessionHandle:
        """Queue one dialogue.  ValueError: a prompt whose context (prompt + step limit + 8) does not fit max_context - nothing is clipped -,
        injected noise or a seed in the wrong kind of session."""
        self.validate(req)
        if self.device_noise and req.noise_seed is None:
            req.noise_seed = int(torch.randint(0, 2 ** 62, (1,)))
        if self.seeded_tokens:
            if req.sampler is None:
                req.sampler = self.default_row
            if req.token_seed is None:
                req.token_seed = int(torch.randint(0, 2 ** 62, (1,)))
        h = SessionHandle(req)
        self.queue.append(h)
        return h

    # ---- chunk delivery and retirement ------------------------------------------------------------------------------
    def _deliver(self, only: Optional[_Dialogue] = None):
        """the staged chunks go to their requests' streamers (only: those of one dialogue - it leaves, the others' wait for the next decode)"""
        keep = []
        for d, b, k in self.pending:
            if only is not None and d is not only:
                keep.append((d, b, k))
                continue
            d.req.audio_streamer.put(self.driver.take_chunk(b, k)[None, None], torch.tensor([0]))      # as run puts them: [samples, 1, T], sample indices
        self.pending[:] = keep

    def _retire(self, b: Optional[int], d: _Dialogue, eos: bool = False):
        """The dialogue leaves: run's finish() (on EOS / its step limit) and run's epilogue for a batch of one."""
        if eos or d.reach:
            self.driver.finished(b)
        self._deliver(only=d)
        if b is not None:
            self.driver.synchronize(b)
            del self.live[b]
        if d.req.audio_streamer is not None:
            d.req.audio_streamer.end()
        r = d.req
        seq = torch.tensor(d.seq, dtype=torch.long)
        rows = [seq if r.head is None or not r.head.numel() else torch.cat([r.head, seq])]
        d.handle._out = pack_output(rows, [torch.cat(d.chunks)[None] if d.chunks else None], [d.reach], self.pad_id, r.in_dev, True)
        d.handle.done = True

    def _stopped(self, d: _Dialogue) -> bool:
        """what ends a dialogue from outside, polled where run polls it: ahead of the dialogue's step"""
        r = d.req
        if d.handle.cancelled:
            return True
        if r.stop_check_fn is not None and r.stop_check_fn():
            if self.verbose:
                print(f"Generation stopped externally at step {d.step + 1}")
            return True
        st = r.audio_streamer
        return st is not None and hasattr(st, "finished_flags") and any(st.finished_flags)      # its stream was ended by someone else (:441-445)

    # ---- one step ---------------------------------------------------------------------------------------------------
    def _forced(self, d: _Dialogue):
        f = d.req.forced_tokens
        return f[d.step] if (f is not None and d.step < len(f)) else None

    def _eligible(self, d: _Dialogue, sde: bool):
        if not (self.speculate and d.prev_tok == self.special["speech_diffusion"]):
            return None
        if self.device_noise:
            return (d.frame, None)
        nz, snz = d.req.noise, d.req.sde_noise
        if nz is not None and d.frame < len(nz) and (not sde or (snz is not None and d.frame < len(snz))):
            return (nz[d.frame], snz[d.frame] if sde else None)
        return None

    def _handle(self, toks: Dict[int, int], speculated: set):
        """run's per-step token handling (:517-670) for the slots in `toks`, every dialogue on its own step counter"""
        drv, sp = self.driver, self.special
        SE, SD, EOS = sp["speech_end"], sp["speech_diffusion"], sp["eos"]
        sde, diffusing = drv.sde, []
        for b in sorted(toks):
            d, tok = self.live[b], toks[b]
            if b in speculated and tok != SD:
                drv.rollback(b)
                speculated.discard(b)
            d.prev_tok = tok
            d.seq.append(tok)
            if tok == EOS:
                if self.verbose:
                    print(f"Samples [{b}] reached EOS token at step {d.step + 1}.", flush=True)
                self._retire(b, d, eos=True)
                continue
            if d.step >= d.max_steps:                      # :528-537 (a batch of one runs out of steps first; kept as run has it)
                d.reach = True
                self._retire(b, d)
                continue
            if tok == SE:
                drv.reset_speech(b)
            if tok == SD:
                diffusing.append(b)
            else:
                drv.embed(b)
        need = []
        if not self.device_noise:
            need = [b for b in diffusing if b not in speculated and
                    (self.live[b].req.noise is None or self.live[b].frame >= len(self.live[b].req.noise))]
        if need:
            n = len(need)
            drawn = torch.randn(2 * n, self.latent)[:n]
            sdrawn = torch.stack([torch.randn(2 * n, self.latent)[:n] for _ in range(drv.n_steps)], dim=1) if sde else None
        rows = {}
        for b in diffusing:
            d = self.live[b]
            if b in need:
                i = need.index(b)
                rows[b] = (drawn[i], sdrawn[i] if sde else None)
            elif b not in speculated:
                rows[b] = (d.frame, None) if self.device_noise else (d.req.noise[d.frame], d.req.sde_noise[d.frame] if sde else None)
        if diffusing:
            drv.speech(rows)
        for b in diffusing:
            d = self.live[b]
            d.chunks.append(drv.chunk(b))
            if d.req.audio_streamer is not None:
                self.pending.append((d, b, drv.stage_chunk(b)))
            d.frame += 1
        for b in sorted(toks):
            d = self.live.get(b)
            if d is not None:                              # still here: on to its next step
                d.step += 1
                if d.step >= d.max_steps or d.L0 + d.step >= d.max_length:      # run's loop runs out of steps (:452-457 for the length)
                    d.reach = d.reach or d.step < d.max_steps
                    self._retire(b, d)

    def _admit_packed(self) -> List[int]:
        """_admit with packed_prefill: every queued request that finds a free slot is admitted (FIFO, lowest free slot first, driver.admit for
        each as ever), ONE driver.first_tokens call prefills them - the driver packs a row batch's newcomers into one weight pass - and their
        tokens are handled together in slot order, as a decode step's are.  A first token that retires its dialogue frees the slot for whoever still waits: the stages repeat.
        admission_ms holds one entry per such wave (what the running dialogues waited), admissions one per request."""
        drv, new = self.driver, []
        while self.queue and len(self.live) < self.slots:
            t0, wave = time.perf_counter(), []
            while self.queue and len(self.live) < self.slots:
                h = self.queue.pop(0)
                r = h.request
                max_length, max_steps = self.limits_of(int(r.prompt.shape[0]), r.max_new_tokens, r.max_length_times)
                d = _Dialogue(h, max_length, max_steps)
                if self._stopped(d) or max_steps <= 0:
                    self._retire(None, d)
                    continue
                b = min(set(range(self.slots)) - set(self.live))
                self.admissions.append((b, sorted(self.live)))
                h.slot = b
                self.live[b] = d
                drv.admit(b, r)
                wave.append(b)
            if not wave:
                continue
            wave.sort()
            forced = {b: self._forced(self.live[b]) for b in wave}
            kw = {} if self.sampler is None else dict(q={b: draw_q(self.nv) for b in wave if forced[b] is None})
            toks = drv.first_tokens(wave, forced, self.sample_fn, **kw)
            self.admission_ms.append((time.perf_counter() - t0) * 1e3)
            # one _handle for the wave, as a decode step's tokens are handled: slot order, and ONE driver.speech for its diffusing dialogues - a
            # diffusion sampling per newcomer would rewrite every dialogue's latent while the previous newcomer's conv tail still reads its own
            self._handle({b: toks[b] for b in wave}, set())
            new += wave
        return new

    def _admit(self) -> List[int]:
        """returns the slots it filled"""
        if self.packed_prefill:
            return self._admit_packed()
        drv, new = self.driver, []
        while self.queue and len(self.live) < self.slots:
            h = self.queue.pop(0)
            r = h.request
            max_length, max_steps = self.limits_of(int(r.prompt.shape[0]), r.max_new_tokens, r.max_length_times)
            d = _Dialogue(h, max_length, max_steps)
            if self._stopped(d) or max_steps <= 0:
                self._retire(None, d)
                continue
            b = min(set(range(self.slots)) - set(self.live))
            self.admissions.append((b, sorted(self.live)))
            t0 = time.perf_counter()
            h.slot = b
            self.live[b] = d
            drv.admit(b, r)
            forced = {b: self._forced(d)}
            kw = {} if self.sampler is None else dict(q={b: draw_q(self.nv)} if forced[b] is None else {})
            toks = drv.first_tokens([b], forced, self.sample_fn, **kw)
            self.admission_ms.append((time.perf_counter() - t0) * 1e3)
            self._handle({b: toks[b]}, set())
            new.append(b)
        return new

    def step(self) -> bool:
        """Admissions, one decode step of every live dialogue, its tokens and frames.  False once nothing is live or queued."""
        if self.closed:
            return False
        drv = self.driver
        for b in sorted(self.live):                        # who leaves from outside does so ahead of its step, and frees its slot for this step's admissions
            if self._stopped(self.live[b]):
                self._retire(b, self.live[b])
        for h in [h for h in self.queue if h.cancelled]:
            self.queue.remove(h)
            self._retire(None, _Dialogue(h, 0, 0))
        for b in self._admit():                            # a newcomer takes its second step with the others: polled ahead of it like them
            if b in self.live and self._stopped(self.live[b]):
                self._retire(b, self.live[b])
        live = sorted(self.live)
        if live:
            forced = {b: self._forced(self.live[b]) for b in live}
            eligible = {}
            for b in live:
                row = self._eligible(self.live[b], drv.sde)
                if row is not None:
                    eligible[b] = row
            kw = {} if self.sampler is None else dict(q={b: draw_q(self.nv) for b in live if forced[b] is None})
            toks, speculated = drv.decode(live, forced, eligible, self.sample_fn, self._deliver, **kw)
            self._handle({b: toks[b] for b in live}, set(speculated))
        return bool(self.live or self.queue)

    def run(self):
        while self.step():
            pass

    def close(self):
        """Whoever is still live or queued is retired as cancelled (its stream ended, its result what it has so far)."""
        if self.closed:
            return
        for b in sorted(self.live):
            self._retire(b, self.live[b])
        for h in self.queue:
            self._retire(None, _Dialogue(h, 0, 0))
        self.queue = []
        self.driver.synchronize()
        self.closed = True
        if self._on_close is not None:
            self._on_close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
