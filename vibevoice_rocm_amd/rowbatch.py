"""Row-batched decode for the dialogues of ONE generate() call (reference: the batched loop of modeling_vibevoice_inference.py:430-673).

`Engine` lanes run B dialogues as B independent launch chains that each stream every LLM and diffusion-head weight once per frame.  Here the
B dialogues (2 <= B <= 4 per RowBatch, up to 8 on a row_batch_width=8 model; generate() runs more as several of them in one loop) share ONE chain for the two weight-heavy parts of a frame:

  graph A   Qwen2 decode step with R = 2 B rows (dialogue b = rows {2 b: positive, 2 b + 1: negative} of x, lens and one KV cache with 2 B
            rows): every weight matrix is read once for all dialogues (4..8 rows, and 10..16 on bf16 weights: the matrix-core GEMV of csrc/vv_gemv_rows.hip on
            fragment-major weight copies - of the e4m3 codes with weight_quant="fp8", of the MXFP4 codes and scale bytes with weight_quant="mxfp4" and
            mxfp4_row_batch=True (csrc/vv_gemv_rows.hip), MXFP6 ones with mxfp6_row_batch=True (csrc/vv_gemv_rows_mx6.hip)), then vv_llm_tail_batch = final norm, constrained logits, argmax / forced token and position
            bookkeeping per dialogue.  With do_sample it splits as Engine.step_decode does: A1 = the decode step and the constrained logits
            (no position bookkeeping), one host read-back of every row batch's logits, the tokens drawn on the host, A2 = the bookkeeping with
            those tokens as forced tokens;
  graph H   vv_head_sample_batch(_sde): the CFG diffusion sampler for all B utterances, 2 B rows through every head matrix per solver step
            (the SDE solver: with the per-step variance noise of every utterance, uploaded with the initial noise).

The conv tokenizers (acoustic decode, semantic encode) and the connectors stay per dialogue - each has its own streaming state - and run as
B concurrent hipGraphs on the lanes' streams between H and the next A (events fork / join them), exactly the launch sequences the lanes use.
They are enqueued only once H has finished: a lane queue that sits on a cross-stream wait while the main queue runs A and H slows every dependent
launch there.  A serving session (modeling.open_session) keeps a row batch open and refills its slots one by one (`admit`),
with every dialogue's guidance scale on the device (`begin(cfg_rows=)`, graph "Hc": vv_head_sample_batch_cfg).  The host loop, token state machine, speculation and rollback are the one batched loop's (batchloop.run), which drives row batches through
modeling._RowDriver."""
from __future__ import annotations

import ctypes as C
import itertools
import os
from typing import Dict, List, Optional

import torch

from . import _lib as L
from .engine import Engine, write_sampler_row, write_seed_rows

_UID = itertools.count(1)
# One worker thread per HIP stream, shared by every RowBatch of the process: two row batches of one generate() call (5..8 dialogues) put their
# lanes on the same four streams, and a stream must never be fed by two host threads at once (the first use of a graph CAPTURES on the stream).
# _JOBS: every launch handed to a worker and not yet known to be in its stream's queue.
_STREAM_WORKERS: Dict[int, "object"] = {}
_JOBS: List["object"] = []


def _submit(stream: torch.cuda.Stream, fn, *args):
    from concurrent.futures import ThreadPoolExecutor
    w = _STREAM_WORKERS.get(stream.cuda_stream)
    if w is None:
        w = _STREAM_WORKERS[stream.cuda_stream] = ThreadPoolExecutor(max_workers=1)
    _JOBS.append(w.submit(fn, *args))


def _wait_all_jobs():
    while _JOBS:
        _JOBS.pop(0).result()


class ConvRowsBook:
    """Host bookkeeping of the row-batched conv tails (batched_conv_rows): which dialogues owe a "back" - semantic encoder back end and
    connectors into their rows of x - and which mask every call uploads.  No device work: RowBatch asks it, tests drive it alone.
    A step may run several fronts (speculated dialogues first, the rest later); the back runs once, in front of the next graph A, over the
    union of the dialogues that still owe one; a rolled-back frame owes nothing."""

    def __init__(self, B: int):
        self.B = int(B)
        self.owed: set = set()
        self.log: List[tuple] = []          # ("front" | "back", mask) per uploaded mask, in order

    def _mask(self, which) -> List[int]:
        w = set(int(b) for b in which)
        if not w <= set(range(self.B)):
            raise ValueError(f"dialogues {sorted(w)} of a row batch of {self.B}")
        return [1 if b in w else 0 for b in range(self.B)]

    def front(self, which) -> List[int]:
        """a speech call for `which`: its front's mask; they now owe a back"""
        m = self._mask(which)
        if not any(m):
            raise ValueError("a front without a dialogue")
        self.owed |= set(int(b) for b in which)
        self.log.append(("front", tuple(m)))
        return m

    def rollback(self, b: int):
        """dialogue b's frame was mis-speculated: its state is restored, it owes nothing"""
        self.owed.discard(int(b))

    def back(self) -> Optional[List[int]]:
        """in front of graph A: the mask of the one back of this step, or None when nobody owes one"""
        if not self.owed:
            return None
        m = self._mask(self.owed)
        self.owed = set()
        self.log.append(("back", tuple(m)))
        return m

    def restart(self):
        """a fresh batch (RowBatch.begin): nobody owes anything"""
        self.owed = set()


def row_batch_ok(quant, mxfp4_row_batch: bool = False, mxfp6_row_batch: bool = False) -> bool:
    """Does the row-batched decode step serve weights of this weight_quant?  bf16 and weight-only fp8 as they are; MXFP4 / MXFP6 with their
    fragment-major opt-in (DeviceWeights.ensure_frag builds the copies the 3..8-row kernels stream); NF4 never."""
    return quant in (None, "fp8") or (quant == "mxfp4" and bool(mxfp4_row_batch)) or (quant == "mxfp6" and bool(mxfp6_row_batch))


class RowBatch:
    def __init__(self, lanes: List[Engine], stream: Optional[torch.cuda.Stream] = None):
        """lanes: one Engine per dialogue (conv state, conv graphs, its stream).  stream: the stream graphs A and H run on (default: lanes[0]'s);
        a lane whose stream IS that stream runs its conv tail inline behind H, the others fork / join through events."""
        self.lanes = lanes
        self.B = B = len(lanes)
        if not 2 <= B <= 8:
            raise L.VVError("row batching serves 2..8 dialogues per row batch")
        eng = self.main = lanes[0]
        self.lib, self.cfg, self.device, self.stream = eng.lib, eng.cfg, eng.device, (stream or eng.stream)
        self._on_main = [e.stream.cuda_stream == self.stream.cuda_stream for e in lanes]
        if eng.dtype != torch.bfloat16 or eng.kv_dtype != torch.bfloat16 or getattr(eng, "kv_fp8", False) or \
                not row_batch_ok(eng.w.quant, eng.w.mxfp4_row_batch, eng.w.mxfp6_row_batch):
            raise L.VVError("row batching needs bf16 weights (or their weight-only fp8 companions, or MXFP4 / MXFP6 ones with mxfp4_row_batch=True / "
                            "mxfp6_row_batch=True) and a bf16 KV cache "
                            "(kv_cache_dtype='fp8' batches run on the lanes: the row-batched decode step has no fp8-KV form)")
        if B > 4 and eng.w.quant is not None:
            raise L.VVError("row batches of 5..8 dialogues (10..16 rows) need bf16 weights without companions: the 16-row matrix-core GEMV has no quantized form")
        self.uid = next(_UID)
        cfg, H = self.cfg, self.cfg.hidden
        f32 = dict(dtype=torch.float32, device=self.device)
        i32 = dict(dtype=torch.int32, device=self.device)
        with torch.cuda.stream(self.stream):
            eng.w.ensure_frag()
            self.x = torch.zeros(2 * B, H, **f32)
            self.hidden = torch.zeros(2 * B, H, **f32)
            self.lens = torch.zeros(2 * B, **i32)
            self.frame_ctr = torch.zeros(B, **i32)
            self.token_dev = torch.zeros(B, **i32)
            self.forced_dev = torch.full((B,), -1, **i32)
            self.active_dev = torch.ones(B, **i32)
            self.logits = torch.zeros(B, 8, **f32)
            self.logits_host = torch.zeros(B, 8, dtype=torch.float32).pin_memory()
            self.q_dev = torch.ones(B, 8, **f32)          # device-side do_sample: every dialogue's exponential draws of the step
            self.noise_dev = torch.zeros(B, cfg.latent, **f32)
            self.noise_seed_dev = torch.zeros(B, dtype=torch.int64, device=self.device)      # device noise: every dialogue's 64-bit seed (its bits)
            self.noise_frame_dev = torch.zeros(B, **i32)                                       # and the index of the frame it draws next
            self.latent = torch.zeros(B, cfg.latent, **f32)
            self.sampler_dev = torch.zeros(B, 3, **f32)   # seeded token draws: every dialogue's vv_sampler row and 64-bit token seed, read by
            self.tok_seed_dev = torch.zeros(B, dtype=torch.int64, device=self.device)         # its block of the step tail (graph "Ar")
            self.cfg_dev = torch.ones(B, **f32)           # guidance per dialogue, read on the device (begin(cfg_rows=) / admit): graph "Hc"
            self._llm_ws = torch.empty(self.lib.vv_llm_ws_bytes(C.byref(eng.w.llm), 2 * B), dtype=torch.uint8, device=self.device)
        self.conv_rows: Optional[ConvRowsBook] = None      # enable_conv_rows(): the one-row stage of both tokenizers runs once per row batch
        self._pf_ws = None
        self._pf_rows = 0
        self.prefill_passes = 0         # vv_llm_prefill_packed calls so far (prefill_packed)
        self._pk_host = None
        self.token_host = torch.zeros(B, dtype=torch.int32).pin_memory()
        self.forced_host = torch.full((B,), -1, dtype=torch.int32).pin_memory()
        self.active_host = torch.ones(B, dtype=torch.int32).pin_memory()
        self.noise_host = torch.zeros(2, B, cfg.latent, dtype=torch.float32).pin_memory()
        self._noise_k = 0
        self.noise_seed_host = torch.zeros(B, dtype=torch.int64).pin_memory()
        self.noise_frame_host = torch.zeros(2, B, dtype=torch.int32).pin_memory()      # double-buffered like the noise rows
        self._frame_k = 0
        self.cfg_host = torch.ones(B, dtype=torch.float32).pin_memory()
        self.cfg_rows = False           # this batch's graph H reads cfg_dev (vv_head_sample_batch_cfg) instead of taking cfg_scale as a launch argument
        self.q_host = torch.ones(2, B, 8, dtype=torch.float32).pin_memory()
        self._q_k = 0
        self._sampler, self._sampler_key = None, None
        self.sampler_host = torch.zeros(B, 3, dtype=torch.float32).pin_memory()
        self.sampler_host[:, 2] = 1.0                     # greedy rows: (0, 0, 1)
        self.tok_seed_host = torch.zeros(B, dtype=torch.int64).pin_memory()
        self._sampler_rows = [(0.0, 0, 1.0)] * B
        self._seeded = False            # set_token_seeds / admit(sampler=): the batch draws its tokens from (token seed, position) - graph "Ar"
        self._forced_val = [-1] * B
        self._active_val = [1] * B
        self._tok_event = torch.cuda.Event()
        self._head_event = torch.cuda.Event()
        self._lane_event = [torch.cuda.Event() for _ in range(B)]
        self._lane_dirty = [False] * B      # lane b has work in flight that the next graph A must wait for
        # the conv tails go out from one worker thread per lane stream (a hipGraph launch costs the host ~0.08 ms: four in a row would delay the
        # last tail by a quarter of a millisecond; the HIP calls release the GIL), see _STREAM_WORKERS
        self.late_tails = os.environ.get("VV_RB_LATE_TAILS", "1") != "0"
        self._timing = [] if os.environ.get("VV_RB_TIMING") else None      # debug: per-step HIP events (A start / A end / H end / tails end)
        self._tcur = None
        self.kv = None
        self._kv_t = None
        self._graphs: Dict[tuple, int] = {}
        self._head_ws = None
        self._head_temb = None          # the lane's t_embedder table the head workspace / noise buffers were sized for (a new one on any set_steps)
        self.sde = False
        self.sde_noise_dev = None
        self.sde_noise_host = None
        self.valid_ids: List[int] = []
        self._w_valid = None
        self._ids_dev = None

    # -----------------------------------------------------------------------------------------------------------------
    @property
    def sp(self) -> int:
        return self.stream.cuda_stream

    def _ck(self, rc, what):
        L.check(rc, what)

    def _drop_graphs(self):
        for g in self._graphs.values():
            self.lib.vv_graph_destroy(g)
        self._graphs = {}

    def close(self):
        self._wait_jobs()
        self._drop_graphs()

    def flush(self):
        """every launch handed to the worker threads is in its stream's queue"""
        self._wait_jobs()

    def _wait_jobs(self):
        _wait_all_jobs()

    def _run(self, name: str, fn, *args):
        if not self.main.use_graphs:
            fn(*args)
            return
        key = (name,) + tuple(args)
        g = self._graphs.get(key)
        if g is None:
            _wait_all_jobs()          # no worker may be waiting on an event of this stream while it captures (another row batch's tails)
            self.stream.synchronize()
            self._ck(self.lib.vv_graph_begin(self.sp), "graph begin")
            try:
                fn(*args)
            finally:
                ge = C.c_void_p()
                rc = self.lib.vv_graph_end(self.sp, C.byref(ge))
            self._ck(rc, "graph end")
            g = ge.value
            self._graphs[key] = g
        self._ck(self.lib.vv_graph_launch(g, self.sp), "graph launch")

    # -----------------------------------------------------------------------------------------------------------------
    def begin(self, s_max: int, valid_ids: List[int], cfg_scale: float, cfg_rows: Optional[List[float]] = None):
        """Fresh batch: one KV cache with 2 B rows sized for s_max tokens, every lane's conv state zeroed.  cfg_rows: one guidance scale per
        dialogue, kept on the device - the batch then runs the graph H whose key has no scale in it (cfg_scale is not used)."""
        cfg, eng, B = self.cfg, self.main, self.B
        s_max = (int(s_max) + 63) // 64 * 64
        self.cfg_scale = float(cfg_scale)
        self.cfg_rows = cfg_rows is not None
        self._seeded = False
        if self.cfg_rows:
            if len(cfg_rows) != B:
                raise L.VVError(f"RowBatch.begin: {len(cfg_rows)} guidance scales for {B} dialogues")
            for b, c in enumerate(cfg_rows):
                self.cfg_host[b] = float(c)
            with torch.cuda.stream(self.stream):
                self.cfg_dev.copy_(self.cfg_host, non_blocking=True)
        for b, e in enumerate(self.lanes):
            if not self._on_main[b]:
                e.sync_in()
                e.stream.wait_stream(self.stream)
        with torch.cuda.stream(self.stream):
            if self.kv is None or self.kv.s_max < s_max:
                shape = (cfg.layers, 2 * B, cfg.kv_heads, s_max, cfg.head_dim)
                self._kv_t = (torch.zeros(shape, dtype=torch.bfloat16, device=self.device), torch.zeros(shape, dtype=torch.bfloat16, device=self.device))
                kv = L.KV()
                kv.k, kv.v = self._kv_t[0].data_ptr(), self._kv_t[1].data_ptr()
                if cfg.head_dim == 128:
                    self._kv_vt = torch.empty((cfg.layers, 2 * B, cfg.kv_heads, s_max // 32, cfg.head_dim, 32), dtype=torch.bfloat16, device=self.device)
                    kv.vt = self._kv_vt.data_ptr()
                kv.kvdt = L.VV_BF16
                kv.layers, kv.rows, kv.kv_heads, kv.s_max, kv.head_dim = cfg.layers, 2 * B, cfg.kv_heads, s_max, cfg.head_dim
                self.kv = kv
                self._drop_graphs()
            ids = sorted(set(int(i) for i in valid_ids))
            if ids != self.valid_ids:
                if len(ids) > 8:
                    raise L.VVError("row batching serves at most 8 constrained vocabulary ids")
                self.valid_ids = ids
                arr = (C.c_int * len(ids))(*ids)
                self._w_valid = torch.empty(len(ids), cfg.hidden, dtype=torch.bfloat16, device=self.device)
                self._ck(self.lib.vv_gather_rows(eng.w.lm_head.data_ptr(), eng.w.wdt, cfg.hidden, arr, len(ids), self._w_valid.data_ptr(), self.sp), "vv_gather_rows")
                self._ids_dev = torch.tensor(ids, dtype=torch.int32, device=self.device)
                self._drop_graphs()
            if self._head_temb is not eng.temb:
                # a new schedule (step count or solver): graph H captured the old t_embedder table, coefficients and buffers
                self.sde = eng.sde
                ws_bytes = (self.lib.vv_head_ws_bytes_batch_sde if self.sde else self.lib.vv_head_ws_bytes_batch)(C.byref(eng.w.head), eng.n_steps, B)
                self._head_ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
                if self.sde:
                    self.sde_noise_dev = torch.zeros(B, eng.n_steps, cfg.latent, dtype=torch.float32, device=self.device)
                    self.sde_noise_host = torch.zeros(2, B, eng.n_steps, cfg.latent, dtype=torch.float32).pin_memory()
                else:
                    self.sde_noise_dev = self.sde_noise_host = None
                self._head_temb = eng.temb
                self._drop_graphs()
            self.lens.zero_()
            self.frame_ctr.zero_()
            self.forced_dev.fill_(-1)
            self.active_dev.fill_(1)
            self.forced_host.fill_(-1)      # the pinned mirrors are uploaded WHOLE whenever one entry changes: they must not carry the last call's values
            self.active_host.fill_(1)
            self._forced_val = [-1] * B
            self._active_val = [1] * B
        for e in self.lanes:
            with torch.cuda.stream(e.stream):
                e.reset_speech_caches()
        self._lane_dirty = [False] * B
        if self.conv_rows is not None:
            self.conv_rows.restart()
            for b in range(B):          # a front on the main stream must see the resets of the lanes' streams
                self._lane_done(b)

    def admit(self, b: int, cfg_scale: float, noise_seed: Optional[int] = None, sampler: Optional[tuple] = None, token_seed: Optional[int] = None):
        """Slot b starts afresh for a new dialogue while the other slots go on (sessions; begin(cfg_rows=) opened the batch): lane b's outstanding
        work is awaited, its positions, frame counter and noise frame index go to zero, forced = none, active, its conv state is zeroed as
        begin zeroes every lane's, and its guidance scale (and noise seed) are written.  sampler = (temperature, top_k, top_p) with token_seed: the
        slot's own warpers and token seed (seeded token draws: the batch then runs graph "Ar").  No other slot's state is touched and no graph is dropped.
        K / V / vt rows the previous occupant left beyond the new positions are never read: attention covers [0, lens] of a row."""
        if not self.cfg_rows:
            raise L.VVError("RowBatch.admit: the batch was not begun with cfg_rows (its graph H has the scale baked in)")
        self._wait_jobs()
        e = self.lanes[b]
        e.stream.synchronize()
        self._lane_dirty[b] = False
        self.cfg_host[b] = float(cfg_scale)
        if noise_seed is not None:
            v = int(noise_seed) & (2 ** 64 - 1)
            self.noise_seed_host[b] = v - 2 ** 64 if v >= 2 ** 63 else v
        self.noise_frame_host[:, b] = 0
        if sampler is not None:
            if token_seed is None:
                raise L.VVError("RowBatch.admit: sampler= needs token_seed=")
            self._sampler_rows[b] = write_sampler_row(self.sampler_host, b, *sampler)
            v = int(token_seed) & (2 ** 64 - 1)
            self.tok_seed_host[b] = v - 2 ** 64 if v >= 2 ** 63 else v
            self._seeded = True
        with torch.cuda.stream(self.stream):
            if sampler is not None:
                self.sampler_dev.copy_(self.sampler_host, non_blocking=True)
                self.tok_seed_dev.copy_(self.tok_seed_host, non_blocking=True)
            self.lens[2 * b: 2 * b + 2].zero_()
            self.frame_ctr[b: b + 1].zero_()
            self.noise_frame_dev[b: b + 1].zero_()
            self.cfg_dev.copy_(self.cfg_host, non_blocking=True)
            if noise_seed is not None:
                self.noise_seed_dev.copy_(self.noise_seed_host, non_blocking=True)
            self._set_forced({b: None})
        self.set_active(b, True)
        with torch.cuda.stream(e.stream):
            e.reset_speech_caches()
            if self.conv_rows is not None:
                self.conv_rows.rollback(b)      # (nothing is owed by a slot that finished; a front waits for the reset through the lane's event)
                self._lane_done(b)

    def prefill(self, b: int, embeds: torch.Tensor, neg: bool = False, chunk: int = 1024, neg_embed: Optional[torch.Tensor] = None, prefix=None):
        """Prompt prefill of dialogue b on cache row 2 b (neg: 2 b + 1), on the main stream; hidden[row] = last hidden state.  neg_embed [1, H]:
        the negative branch's one-token prompt rides along as one more row of the last chunk (cache row 2 b + 1, position 0; Engine.prefill);
        `commit_negative` then puts the branch in use.  prefix (a VoicePrefix): restored into slots [0, P) of row 2 b with one vv_kv_copy, `embeds`
        - the rows after it - prefilled at position P (Engine.prefill)."""
        if prefix is not None and neg:
            raise L.VVError("RowBatch.prefill: a prefix belongs to the positive row")
        row = 2 * b + (1 if neg else 0)
        L0 = embeds.shape[0]
        P = 0 if prefix is None else int(prefix.P)
        n_chunks = max(1, -(-L0 // max(1, chunk)))
        size = -(-L0 // n_chunks)
        size = min(chunk, (size + 31) // 32 * 32) if n_chunks > 1 else L0
        with torch.cuda.stream(self.stream):
            if max(size, 1) + 1 > self._pf_rows:
                self._pf_rows = max(size + 1, 64)
                self._pf_ws = torch.empty(self.lib.vv_llm_ws_bytes(C.byref(self.main.w.llm), self._pf_rows), dtype=torch.uint8, device=self.device)
            if prefix is not None:
                self._ck(self.lib.vv_kv_copy(C.byref(prefix.kv), 0, C.byref(self.kv), row, P, self.sp), "vv_kv_copy")
            for c0 in range(0, L0, size):
                c1 = min(L0, c0 + size)
                last = c1 == L0 and neg_embed is not None
                n = c1 - c0 + (1 if last else 0)
                lens = torch.arange(P + c0, P + c0 + n, dtype=torch.int32, device=self.device)
                rows = torch.full((n,), row, dtype=torch.int32, device=self.device)
                xe = embeds[c0:c1].contiguous()
                if last:
                    lens[-1] = 0
                    rows[-1] = 2 * b + 1
                    xe = torch.cat([xe, neg_embed.to(xe.dtype).reshape(1, -1)])
                out = torch.empty(n, self.cfg.hidden, dtype=torch.float32, device=self.device)
                self._ck(self.lib.vv_llm_forward(C.byref(self.main.w.llm), C.byref(self.kv), xe.data_ptr(), xe.stride(0), n, lens.data_ptr(), rows.data_ptr(),
                                                 out.data_ptr(), out.stride(0), self._pf_ws.data_ptr(), self.sp), "vv_llm_forward")
            if neg_embed is not None:
                self.hidden[row].copy_(out[-2])
                self.hidden[2 * b + 1].copy_(out[-1])
            else:
                self.hidden[row].copy_(out[-1])
            self.lens[row] = P + L0

    def prefill_packed(self, items, chunk_rows: int = 4096, neg_embed: Optional[torch.Tensor] = None):
        """Prompt prefill of SEVERAL dialogues in one weight pass (vv_llm_prefill_packed).  items: [(dialogue b, embeds [L_b, H] of the rows to
        prefill, its VoicePrefix or None)].  Prefixes are restored with vv_kv_copy as `prefill` restores them; the dialogues' rows are packed
        back to back in ascending b - dialogue b on cache row 2 b at positions P_b + i - and cut into passes of at most chunk_rows rows (a cut
        inside a dialogue: its later rows run in the next pass at their own positions, as a chunked prefill's do).  neg_embed [1, H]: every
        dialogue's one-token negative prompt (cache row 2 b + 1, position 0) rides on the last pass; `commit_negative` puts it in use.  Positions,
        cache rows and the selected rows (each dialogue's last, the negatives) are built on the host and uploaded once per pass.  Then hidden[2 b],
        hidden[2 b + 1] and lens[2 b] are what `prefill` leaves.  Counts its passes in self.prefill_passes."""
        items = sorted(items, key=lambda it: it[0])
        if not items or len({it[0] for it in items}) != len(items) or not all(0 <= it[0] < self.B for it in items):
            raise L.VVError("RowBatch.prefill_packed: one entry per dialogue of this row batch")
        chunk_rows, H, nb = max(1, int(chunk_rows)), self.cfg.hidden, len(items)
        pos, row, end = [], [], {}                 # per packed row: position, cache row; index of a dialogue's last row -> its hidden row
        for b, emb, prefix in items:
            P = 0 if prefix is None else int(prefix.P)
            n = int(emb.shape[0])
            if n < 1:
                raise L.VVError("RowBatch.prefill_packed: a dialogue without rows")
            pos += range(P, P + n)
            row += [2 * b] * n
            end[len(pos) - 1] = 2 * b
        T = len(pos)
        cuts = list(range(0, T, chunk_rows))
        if neg_embed is not None:
            pos += [0] * nb
            row += [2 * b + 1 for b, _, _ in items]
            end.update({T + i: 2 * b + 1 for i, (b, _, _) in enumerate(items)})
        passes = [(c0, min(T, c0 + chunk_rows) if i + 1 < len(cuts) else len(pos)) for i, c0 in enumerate(cuts)]
        cap = max(c1 - c0 for c0, c1 in passes)
        # one pinned int32 image per pass: positions | cache rows | selected rows, then (hidden row of each selected row); the last image
        # carries the dialogues' new lens entries behind it: (2 b, P_b + L_b)
        width = 3 * cap + 2 * self.B + 2 * nb
        if self._pk_host is None or self._pk_host.shape[0] < len(passes) or self._pk_host.shape[1] < width:
            self._pk_host = torch.zeros(max(len(passes), 4), width, dtype=torch.int32).pin_memory()
            self._pk_event = torch.cuda.Event()
        else:
            self._pk_event.synchronize()          # the previous call's uploads have left the buffer
        with torch.cuda.stream(self.stream):
            xs = [emb.to(torch.float32) for _, emb, _ in items]
            if neg_embed is not None:
                xs += [neg_embed.to(torch.float32).reshape(1, H)] * nb
            x = torch.cat(xs) if len(xs) > 1 else xs[0].contiguous()
            if cap > self._pf_rows:              # one workspace for `prefill` and the packed passes: the two size functions agree
                self._pf_rows = max(cap, 64)
                self._pf_ws = torch.empty(self.lib.vv_llm_prefill_packed_ws_bytes(C.byref(self.main.w.llm), self._pf_rows), dtype=torch.uint8, device=self.device)
            for b, _, prefix in items:
                if prefix is not None:
                    self._ck(self.lib.vv_kv_copy(C.byref(prefix.kv), 0, C.byref(self.kv), 2 * b, int(prefix.P), self.sp), "vv_kv_copy")
            for p, (c0, c1) in enumerate(passes):
                n = c1 - c0
                sel = [i for i in range(c0, c1) if i in end]
                dst = [end[i] for i in sel]
                if not sel:
                    sel = [c1 - 1]                 # a pass that ends no dialogue: the entry wants a row; its state is dropped
                img = self._pk_host[p]
                img[:n] = torch.tensor(pos[c0:c1], dtype=torch.int32)
                img[cap: cap + n] = torch.tensor(row[c0:c1], dtype=torch.int32)
                img[2 * cap: 2 * cap + len(sel)] = torch.tensor([i - c0 for i in sel], dtype=torch.int32)
                used = 3 * cap + len(dst)
                if dst:
                    img[3 * cap: used] = torch.tensor(dst, dtype=torch.int32)
                last = p + 1 == len(passes)
                if last:
                    img[used: used + 2 * nb] = torch.tensor([2 * b for b, _, _ in items] + [(0 if pf is None else int(pf.P)) + int(emb.shape[0]) for _, emb, pf in items],
                                                            dtype=torch.int32)
                meta = img[: used + (2 * nb if last else 0)].to(self.device, non_blocking=True)
                out = torch.empty(len(sel), H, dtype=torch.float32, device=self.device)
                self._ck(self.lib.vv_llm_prefill_packed(C.byref(self.main.w.llm), C.byref(self.kv), x[c0:c1].data_ptr(), x.stride(0), n, meta.data_ptr(),
                                                        meta[cap:].data_ptr(), meta[2 * cap:].data_ptr(), len(sel), out.data_ptr(), out.stride(0),
                                                        self._pf_ws.data_ptr(), self.sp), "vv_llm_prefill_packed")
                self.prefill_passes += 1
                if dst:
                    self.hidden.index_copy_(0, meta[3 * cap: used].long(), out[: len(dst)])
                if last:
                    self.lens.index_copy_(0, meta[used: used + nb].long(), meta[used + nb: used + 2 * nb])
            self._pk_event.record(self.stream)

    def commit_negative(self, b: int):
        with torch.cuda.stream(self.stream):
            self.lens[2 * b + 1] = 1

    def set_sampler(self, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
        """The warpers of the device-side token draw (Engine.set_sampler)."""
        self._sampler_key = (float(temperature), int(top_k), float(top_p))
        self._sampler = L.Sampler(*self._sampler_key)

    def set_sampler_row(self, b: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0):
        """Seeded token draws: dialogue b's own warpers, kept on the device (Engine.set_sampler_row); greedy = (0, 0, 1)."""
        self._sampler_rows[b] = write_sampler_row(self.sampler_host, b, temperature, top_k, top_p)
        with torch.cuda.stream(self.stream):
            self.sampler_dev.copy_(self.sampler_host, non_blocking=True)

    def set_token_seeds(self, seeds: List[int]):
        """Seeded token draws: the B dialogues' 64-bit token seeds, once per batch (after begin).  decode_begin then runs graph "Ar" - every
        dialogue's token drawn in its block of the tail from (its seed, its position, its logits) under its own sampler row - and takes no q."""
        write_seed_rows(self.tok_seed_host, seeds)
        with torch.cuda.stream(self.stream):
            self.tok_seed_dev.copy_(self.tok_seed_host, non_blocking=True)
        self._seeded = True

    def set_noise_seeds(self, seeds: List[int]):
        """Device noise: the B dialogues' 64-bit seeds, once per batch (after begin); speech / speech_begin given `frames` then draw the noise of
        every row inside graph H (Engine.set_noise_seed)."""
        for b, sd in enumerate(seeds):
            v = int(sd) & (2 ** 64 - 1)
            self.noise_seed_host[b] = v - 2 ** 64 if v >= 2 ** 63 else v
        with torch.cuda.stream(self.stream):
            self.noise_seed_dev.copy_(self.noise_seed_host, non_blocking=True)

    def _upload_q(self, q: Dict[int, torch.Tensor]):
        """{dialogue: its exponential draws [nv]} -> q_dev through a pinned double-buffered [B][8] row (the other dialogues' rows are not read
        for a choice that counts: they are forced or finished)"""
        if self._sampler is None:
            raise L.VVError("device-side sampling needs set_sampler() first")
        self._q_k ^= 1
        qh = self.q_host[self._q_k]
        for b, row in q.items():
            qh[b, : row.numel()].copy_(row.reshape(-1))
        self.q_dev.copy_(qh, non_blocking=True)

    def first_token(self, b: int, forced: Optional[int], sample_fn=None, q=None) -> int:
        """Token selection right after the prefill of dialogue b (hidden[2 b] holds its last prompt state).  With `sample_fn(logits, ids) -> token`
        (do_sample) the constrained logits are read back and the drawn token is selected as a forced one (Engine.first_token); with `q` (the
        dialogue's exponential draws [nv]) the token is drawn on the device (vv_sample_ids)."""
        nv = len(self.valid_ids)
        with torch.cuda.stream(self.stream):
            a = L.LinArgs()
            a.x, a.ldx, a.m = self.hidden[2 * b].data_ptr(), self.cfg.hidden, 1
            a.w, a.n, a.k, a.wdt = self._w_valid.data_ptr(), nv, self.cfg.hidden, L.VV_BF16
            a.out, a.ldo = self.logits[b].data_ptr(), nv
            self._ck(self.lib.vv_linear(C.byref(a), self.sp), "lm_head")
        if self._seeded and forced is None:
            # seeded token draws: the draws of (the dialogue's seed, the last prompt position = lens[2 b] - 1), then its own sampler's choice
            with torch.cuda.stream(self.stream):
                self._set_forced({b: None})
                if self._sampler_rows[b][0] > 0:
                    self._ck(self.lib.vv_token_draws(self.q_dev[b].data_ptr(), 8, 1, nv, self.tok_seed_dev[b:].data_ptr(), self.lens[2 * b:].data_ptr(), 2, -1,
                                                     self.sp), "vv_token_draws")
                    self._ck(self.lib.vv_sample_ids(self.logits[b].data_ptr(), nv, self._ids_dev.data_ptr(), C.byref(L.Sampler(*self._sampler_rows[b])),
                                                    self.q_dev[b].data_ptr(), self.token_dev[b:].data_ptr(), self.forced_dev[b:].data_ptr(), self.sp), "vv_sample_ids")
                else:
                    self._ck(self.lib.vv_argmax_ids(self.logits[b].data_ptr(), nv, self._ids_dev.data_ptr(), self.token_dev[b:].data_ptr(),
                                                    self.forced_dev[b:].data_ptr(), self.sp), "vv_argmax_ids")
                self.token_host.copy_(self.token_dev, non_blocking=True)
            self.stream.synchronize()
            return int(self.token_host[b])
        if sample_fn is not None and forced is None:
            forced = int(sample_fn(self.read_logits()[b, :nv].clone(), self.valid_ids))
        if q is not None and forced is None:
            with torch.cuda.stream(self.stream):
                self._set_forced({b: None})
                self._upload_q({b: q})
                self._ck(self.lib.vv_sample_ids(self.logits[b].data_ptr(), nv, self._ids_dev.data_ptr(), C.byref(self._sampler), self.q_dev[b].data_ptr(),
                                                self.token_dev[b:].data_ptr(), self.forced_dev[b:].data_ptr(), self.sp), "vv_sample_ids")
                self.token_host.copy_(self.token_dev, non_blocking=True)
            self.stream.synchronize()
            return int(self.token_host[b])
        with torch.cuda.stream(self.stream):
            self._set_forced({b: forced})
            self._ck(self.lib.vv_argmax_ids(self.logits[b].data_ptr(), nv, self._ids_dev.data_ptr(), self.token_dev[b:].data_ptr(),
                                            self.forced_dev[b:].data_ptr(), self.sp), "vv_argmax_ids")
            self.token_host.copy_(self.token_dev, non_blocking=True)
        self.stream.synchronize()
        return int(self.token_host[b])

    # -----------------------------------------------------------------------------------------------------------------
    def _set_forced(self, forced: Dict[int, Optional[int]]):
        """Device-side forced tokens (-1: none), uploaded only when one changes (see Engine._set_forced)."""
        changed = False
        for b, f in forced.items():
            v = -1 if f is None else int(f)
            if v != self._forced_val[b]:
                self._forced_val[b] = v
                self.forced_host[b] = v
                changed = True
        if changed:
            self.forced_dev.copy_(self.forced_host, non_blocking=True)

    def set_active(self, b: int, on: bool):
        """A finished dialogue stays in the row batch (its rows are computed and dropped) but no longer advances its positions."""
        v = 1 if on else 0
        if v != self._active_val[b]:
            self._active_val[b] = v
            self.active_host[b] = v
            with torch.cuda.stream(self.stream):
                self.active_dev.copy_(self.active_host, non_blocking=True)

    def _seq_A(self, tok_start, tok_diff):
        eng, B, H = self.main, self.B, self.cfg.hidden
        nv = len(self.valid_ids)
        self._ck(self.lib.vv_llm_forward(C.byref(eng.w.llm), C.byref(self.kv), self.x.data_ptr(), H, 2 * B, self.lens.data_ptr(), None, None, 0,
                                         self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._ck(self.lib.vv_llm_tail_batch(C.byref(eng.w.llm), self._llm_ws.data_ptr(), H, B, self.hidden.data_ptr(), H, self._w_valid.data_ptr(), nv,
                                            self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(), self.forced_dev.data_ptr(),
                                            self.lens.data_ptr(), tok_start, tok_diff, self.frame_ctr.data_ptr(), self.active_dev.data_ptr(), self.sp),
                 "vv_llm_tail_batch")

    def _seq_AS(self, tok_start, tok_diff, temperature, top_k, top_p):
        """_seq_A with the sampling tail (vv_llm_tail_batch_sample); the warpers are part of the graph's key (Engine._seq_AS)"""
        eng, B, H = self.main, self.B, self.cfg.hidden
        nv = len(self.valid_ids)
        smp = L.Sampler(temperature, top_k, top_p)
        self._ck(self.lib.vv_llm_forward(C.byref(eng.w.llm), C.byref(self.kv), self.x.data_ptr(), H, 2 * B, self.lens.data_ptr(), None, None, 0,
                                         self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._ck(self.lib.vv_llm_tail_batch_sample(C.byref(eng.w.llm), self._llm_ws.data_ptr(), H, B, self.hidden.data_ptr(), H, self._w_valid.data_ptr(), nv,
                                                   self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(), self.forced_dev.data_ptr(),
                                                   self.lens.data_ptr(), tok_start, tok_diff, self.frame_ctr.data_ptr(), self.active_dev.data_ptr(),
                                                   C.byref(smp), self.q_dev.data_ptr(), self.sp), "vv_llm_tail_batch_sample")

    def _seq_Ar(self, tok_start, tok_diff):
        """_seq_A with the seeded tail (vv_llm_tail_batch_sample_rows): block b reads dialogue b's sampler row and token seed from sampler_dev /
        tok_seed_dev and forms its draws from (seed, lens[2 b]); no warpers in the graph's key, greedy and sampled dialogues side by side"""
        eng, B, H = self.main, self.B, self.cfg.hidden
        nv = len(self.valid_ids)
        self._ck(self.lib.vv_llm_forward(C.byref(eng.w.llm), C.byref(self.kv), self.x.data_ptr(), H, 2 * B, self.lens.data_ptr(), None, None, 0,
                                         self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._ck(self.lib.vv_llm_tail_batch_sample_rows(C.byref(eng.w.llm), self._llm_ws.data_ptr(), H, B, self.hidden.data_ptr(), H, self._w_valid.data_ptr(), nv,
                                                        self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(), self.forced_dev.data_ptr(),
                                                        self.lens.data_ptr(), tok_start, tok_diff, self.frame_ctr.data_ptr(), self.active_dev.data_ptr(),
                                                        self.sampler_dev.data_ptr(), self.tok_seed_dev.data_ptr(), self.sp), "vv_llm_tail_batch_sample_rows")

    def _seq_A1(self):
        """the decode step and the constrained logits of every dialogue; positions stay (lens / frame_counter NULL)"""
        eng, B, H = self.main, self.B, self.cfg.hidden
        self._ck(self.lib.vv_llm_forward(C.byref(eng.w.llm), C.byref(self.kv), self.x.data_ptr(), H, 2 * B, self.lens.data_ptr(), None, None, 0,
                                         self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._ck(self.lib.vv_llm_tail_batch(C.byref(eng.w.llm), self._llm_ws.data_ptr(), H, B, self.hidden.data_ptr(), H, self._w_valid.data_ptr(),
                                            len(self.valid_ids), self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(), None,
                                            None, 0, 0, None, None, self.sp), "vv_llm_tail_batch")

    def _seq_A2(self, tok_start, tok_diff):
        """the tail again on the same rows (deterministic: hidden / logits are rewritten with the same values), now with the drawn tokens forced
        and the position bookkeeping of every live dialogue"""
        eng, B, H = self.main, self.B, self.cfg.hidden
        self._ck(self.lib.vv_llm_tail_batch(C.byref(eng.w.llm), self._llm_ws.data_ptr(), H, B, self.hidden.data_ptr(), H, self._w_valid.data_ptr(),
                                            len(self.valid_ids), self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(),
                                            self.forced_dev.data_ptr(), self.lens.data_ptr(), tok_start, tok_diff, self.frame_ctr.data_ptr(),
                                            self.active_dev.data_ptr(), self.sp), "vv_llm_tail_batch")

    def _seq_H(self, cfg_scale, dn=None):
        """dn == "dn": the noise of all B rows is drawn on the device first, from (noise_seed_dev, noise_frame_dev) - the rows of dialogues that
        do not diffuse are drawn from whatever index they hold and dropped, as their samples are.  The marker is part of the graph's key."""
        eng, cfg = self.main, self.cfg
        if dn:
            self._ck(self.lib.vv_noise_normal(self.noise_dev.data_ptr(), cfg.latent, self.sde_noise_dev.data_ptr() if self.sde else None,
                                              eng.n_steps * cfg.latent, self.B, cfg.latent, eng.n_steps if self.sde else 0,
                                              self.noise_seed_dev.data_ptr(), self.noise_frame_dev.data_ptr(), self.sp), "vv_noise_normal")
        if self.sde:
            self._ck(self.lib.vv_head_sample_batch_sde(C.byref(eng.w.head), self.hidden.data_ptr(), cfg.hidden, self.noise_dev.data_ptr(), cfg.latent,
                                                       eng.temb.data_ptr(), eng._coefs, eng.n_steps, cfg_scale, self.latent.data_ptr(), cfg.latent, self.B,
                                                       self._head_ws.data_ptr(), self.sde_noise_dev.data_ptr(), eng.n_steps * cfg.latent, self.sp),
                     "vv_head_sample_batch_sde")
            return
        self._ck(self.lib.vv_head_sample_batch(C.byref(eng.w.head), self.hidden.data_ptr(), cfg.hidden, self.noise_dev.data_ptr(), cfg.latent,
                                               eng.temb.data_ptr(), eng._coefs, eng.n_steps, cfg_scale, self.latent.data_ptr(), cfg.latent, self.B,
                                               self._head_ws.data_ptr(), self.sp), "vv_head_sample_batch")

    def _seq_Hc(self, dn=None):
        """_seq_H with every dialogue's guidance scale read from cfg_dev (vv_head_sample_batch_cfg): no scale in the graph's key"""
        eng, cfg = self.main, self.cfg
        if dn:
            self._ck(self.lib.vv_noise_normal(self.noise_dev.data_ptr(), cfg.latent, self.sde_noise_dev.data_ptr() if self.sde else None,
                                              eng.n_steps * cfg.latent, self.B, cfg.latent, eng.n_steps if self.sde else 0,
                                              self.noise_seed_dev.data_ptr(), self.noise_frame_dev.data_ptr(), self.sp), "vv_noise_normal")
        self._ck(self.lib.vv_head_sample_batch_cfg(C.byref(eng.w.head), self.hidden.data_ptr(), cfg.hidden, self.noise_dev.data_ptr(), cfg.latent,
                                                   eng.temb.data_ptr(), eng._coefs, eng.n_steps, self.cfg_dev.data_ptr(), self.latent.data_ptr(), cfg.latent,
                                                   self.B, self._head_ws.data_ptr(), self.sde_noise_dev.data_ptr() if self.sde else None,
                                                   eng.n_steps * cfg.latent if self.sde else 0, self.sp), "vv_head_sample_batch_cfg")

    def _run_H(self, dn: bool):
        if self.cfg_rows:
            self._run("Hc", self._seq_Hc, *(("dn",) if dn else ()))
        else:
            self._run("H", self._seq_H, float(self.cfg_scale), *(("dn",) if dn else ()))

    def _seq_conv(self, b, uid):
        """acoustic decode -> semantic encode -> connectors of dialogue b on ITS stream, into rows 2 b, 2 b + 1 of the next step's input"""
        e, cfg = self.lanes[b], self.cfg
        lib, w = self.lib, e.w
        blob = w.state_blob()
        self._ck(lib.vv_copy_rows(blob.data_ptr(), blob.numel(), e._state_snap.data_ptr(), blob.numel(), 1, blob.numel(), e.sp), "snapshot")
        lat = self.latent[b].data_ptr()
        self._ck(lib.vv_decoder_forward(C.byref(w.dec), lat, 1, 1.0 / w.speech_scale, -w.speech_bias, e.wav.data_ptr(), e._dec_ws.data_ptr(), e.sp),
                 "vv_decoder_forward")
        self._ck(lib.vv_encoder_forward(C.byref(w.sem), e.wav.data_ptr(), cfg.hop, e.sem.data_ptr(), e._sem_ws.data_ptr(), e.sp), "vv_encoder_forward")
        self._ck(lib.vv_connector_pair(C.byref(w.ac_conn), C.byref(w.sem_conn), lat, e.sem.data_ptr(), self.x[2 * b].data_ptr(), cfg.hidden, 2,
                                       e.conn_ws.data_ptr(), e.sp), "connectors")

    # ---- batched_conv_rows: front (main stream) -> middles (lanes) -> back (main stream, in front of the next graph A) ----------------
    def enable_conv_rows(self):
        """Switch this row batch to the row-batched conv tails (vv_decoder_front_rows / vv_encoder_back_rows / vv_connector_pair_rows): the
        one-row stage of both tokenizers reads its weights once for all dialogues.  Idempotent; the per-dialogue tail graphs are not touched."""
        if self.conv_rows is not None:
            return
        eng, cfg, B, lib = self.main, self.cfg, self.B, self.lib
        if eng.w.quant is not None or eng.dtype != torch.bfloat16:
            raise L.VVError("batched_conv_rows needs bf16 weights without companions")
        fb = lib.vv_conv_rows_ws_bytes(C.byref(eng.w.dec), B, 1)
        bb = lib.vv_conv_rows_ws_bytes(C.byref(eng.w.sem), B, 0)
        if not fb or not bb:
            raise L.VVError("batched_conv_rows: the tokenizers' one-row stage is not C = 2048 (n_filters != 32)")
        f32 = dict(dtype=torch.float32, device=self.device)
        self._cr_dec = (C.POINTER(L.ConvNet) * B)(*[C.pointer(e.w.dec) for e in self.lanes])
        self._cr_sem = (C.POINTER(L.ConvNet) * B)(*[C.pointer(e.w.sem) for e in self.lanes])
        with torch.cuda.stream(self.stream):
            self._cr_mid = torch.zeros(B, 8192, **f32)         # front -> middle: the decoder's C = 1024 stage input of every dialogue
            self._cr_mid2 = torch.zeros(B, 8192, **f32)        # middle -> back: the encoder's C = 1024 stage output
            self._cr_feat = torch.zeros(B, cfg.sem_dim, **f32)
            self._cr_lat = torch.zeros(B, cfg.latent, **f32)   # the latents of the dialogues that owe a back (a later graph H rewrites self.latent)
            self._cr_front_ws = torch.empty(fb, dtype=torch.uint8, device=self.device)
            self._cr_back_ws = torch.empty(bb, dtype=torch.uint8, device=self.device)
            self._cr_conn_ws = torch.empty(2 * B * cfg.hidden, **f32)
            self._cr_front_mask = torch.zeros(B, dtype=torch.int32, device=self.device)
            self._cr_back_mask = torch.zeros(B, dtype=torch.int32, device=self.device)
        self._cr_mask_host = torch.zeros(8, B, dtype=torch.int32).pin_memory()     # a ring: a row is rewritten 8 uploads later
        self._cr_mask_k = 0
        self._front_event = torch.cuda.Event()
        self.conv_rows = ConvRowsBook(B)

    def _cr_upload(self, mask: List[int], dev: torch.Tensor):
        self._cr_mask_k = (self._cr_mask_k + 1) % self._cr_mask_host.shape[0]
        row = self._cr_mask_host[self._cr_mask_k]
        for b, v in enumerate(mask):
            row[b] = int(v)
        dev.copy_(row, non_blocking=True)

    def _seq_front(self):
        w = self.main.w
        self._ck(self.lib.vv_decoder_front_rows(self._cr_dec, self.B, self._cr_front_mask.data_ptr(), self.latent.data_ptr(), self.cfg.latent,
                                                1.0 / w.speech_scale, -w.speech_bias, self._cr_mid.data_ptr(), self._cr_mid.stride(0),
                                                self._cr_front_ws.data_ptr(), self.sp), "vv_decoder_front_rows")

    def _seq_mid(self, b, uid):
        """the stages below the one-row stage of dialogue b on ITS stream: decoder from its hand-over rows, encoder up to its hand-over rows"""
        e, cfg, lib = self.lanes[b], self.cfg, self.lib
        self._ck(lib.vv_decoder_forward_from(C.byref(e.w.dec), self._cr_mid[b].data_ptr(), e.wav.data_ptr(), e._dec_ws.data_ptr(), e.sp), "vv_decoder_forward_from")
        self._ck(lib.vv_encoder_forward_until(C.byref(e.w.sem), e.wav.data_ptr(), cfg.hop, self._cr_mid2[b].data_ptr(), e._sem_ws.data_ptr(), e.sp),
                 "vv_encoder_forward_until")

    def _seq_back(self):
        w, cfg = self.main.w, self.cfg
        self._ck(self.lib.vv_encoder_back_rows(self._cr_sem, self.B, self._cr_back_mask.data_ptr(), self._cr_mid2.data_ptr(), self._cr_mid2.stride(0),
                                               self._cr_feat.data_ptr(), cfg.sem_dim, self._cr_back_ws.data_ptr(), self.sp), "vv_encoder_back_rows")
        self._ck(self.lib.vv_connector_pair_rows(C.byref(w.ac_conn), C.byref(w.sem_conn), self._cr_lat.data_ptr(), cfg.latent, self._cr_feat.data_ptr(),
                                                 cfg.sem_dim, self._cr_back_mask.data_ptr(), self.x.data_ptr(), cfg.hidden, 2, self.B,
                                                 self._cr_conn_ws.data_ptr(), self.sp), "vv_connector_pair_rows")

    def _back_if_owed(self):
        """on the main stream, after _join_lanes and in front of graph A: the one back of the step for the dialogues that owe one"""
        if self.conv_rows is None:
            return
        mask = self.conv_rows.back()
        if mask is None:
            return
        self._cr_upload(mask, self._cr_back_mask)
        self._run("back", self._seq_back)

    def _speech_tails_rows(self, which: List[int]):
        """speech_tails with batched_conv_rows: snapshots + front on the main stream right behind H, then every dialogue's middle on its lane"""
        late = self.late_tails
        with torch.cuda.stream(self.stream):
            self._join_lanes()          # reset_speech / rollback / embed ran on the lanes' streams: the front reads and writes their state
            mask = self.conv_rows.front(which)
            for b in which:             # the rollback snapshot of every active dialogue, before the front writes any state; and its latent
                e = self.lanes[b]
                blob = e.w.state_blob()
                self._ck(self.lib.vv_copy_rows(blob.data_ptr(), blob.numel(), e._state_snap.data_ptr(), blob.numel(), 1, blob.numel(), self.sp), "snapshot")
                self._ck(self.lib.vv_copy_rows(self.latent[b].data_ptr(), self.cfg.latent, self._cr_lat[b].data_ptr(), self.cfg.latent, 1, self.cfg.latent,
                                               self.sp), "latent")
            self._cr_upload(mask, self._cr_front_mask)
            self._run("front", self._seq_front)
            self._front_event.record(self.stream)

        def mid(b):
            e = self.lanes[b]
            torch.cuda.set_device(self.device)
            if late and not self._on_main[b]:
                self._front_event.synchronize()     # the worker waits for the front as a late tail waits for H: no stream-side wait
            with torch.cuda.stream(e.stream):
                e._run("RBmid", self._seq_mid, b, self.uid)
                self._lane_done(b)
                if self._timing is not None and self._tcur is not None:
                    ev = torch.cuda.Event(enable_timing=True)
                    ev.record(e.stream)
                    self._tcur["t"].append(ev)

        inline = []
        for b in which:
            if self._on_main[b]:
                inline.append(b)
            else:
                if not late:
                    self.lanes[b].stream.wait_event(self._front_event)
                _submit(self.lanes[b].stream, mid, b)
        for b in inline:
            e = self.lanes[b]
            if e.use_graphs and ("RBmid", b, self.uid) not in e._graphs:
                _wait_all_jobs()        # first use captures on the main stream: no worker may still be waiting on _front_event (recorded there)
            mid(b)

    def _seq_embed(self, b, uid):
        e, cfg = self.lanes[b], self.cfg
        self._ck(self.lib.vv_embed_row(e.w.embed.data_ptr(), e.w.wdt, cfg.hidden, self.token_dev[b:].data_ptr(), self.x[2 * b].data_ptr(), e.sp), "embed")
        self._ck(self.lib.vv_copy_rows(self.x[2 * b].data_ptr(), 0, self.x[2 * b + 1].data_ptr(), cfg.hidden, 1, cfg.hidden, e.sp), "copy")

    def _join_lanes(self):
        """the next graph A reads every lane's rows of x"""
        self._wait_jobs()
        for b in range(self.B):
            if self._lane_dirty[b]:
                self.stream.wait_event(self._lane_event[b])
                self._lane_dirty[b] = False

    def _lane_done(self, b):
        if not self._on_main[b]:
            self._lane_event[b].record(self.lanes[b].stream)
            self._lane_dirty[b] = True

    def decode_begin(self, tok_start: int, tok_diff: int, forced: Dict[int, Optional[int]], q: Optional[Dict[int, torch.Tensor]] = None):
        """graph A for all dialogues + the asynchronous token read-back; `decode_end` returns the tokens.  `q` = {dialogue: exponential draws
        [nv]} (do_sample on the device): the sampling variant of graph A - a dialogue with a forced token keeps it, the others draw theirs."""
        with torch.cuda.stream(self.stream):
            self._join_lanes()
            self._back_if_owed()
            self._set_forced(forced)
            if self._timing is not None:
                self._tcur = dict(a0=torch.cuda.Event(enable_timing=True), a1=torch.cuda.Event(enable_timing=True), h1=None, t=[])
                self._timing.append(self._tcur)
                self._tcur["a0"].record(self.stream)
            if self._seeded:
                self._run("Ar", self._seq_Ar, int(tok_start), int(tok_diff))
            elif q:
                self._upload_q(q)
                self._run("AS", self._seq_AS, int(tok_start), int(tok_diff), *self._sampler_key)
            else:
                self._run("A", self._seq_A, int(tok_start), int(tok_diff))
            if self._timing is not None:
                self._tcur["a1"].record(self.stream)
            self.token_host.copy_(self.token_dev, non_blocking=True)
            self._tok_event.record(self.stream)

    def decode_end(self) -> List[int]:
        self._tok_event.synchronize()
        return [int(t) for t in self.token_host]

    def decode_logits(self):
        """do_sample, first half: graph A1 for all dialogues + the asynchronous copy of their constrained logits; the caller enqueues this for
        every row batch of the step before it waits for any (`logits_end`), then hands the drawn tokens to `decode_commit`."""
        with torch.cuda.stream(self.stream):
            self._join_lanes()
            self._back_if_owed()
            self._run("A1", self._seq_A1)
            self.logits_host.copy_(self.logits, non_blocking=True)
            self._tok_event.record(self.stream)

    def logits_end(self) -> torch.Tensor:
        """[B][8] constrained logits of the step (row b: dialogue b, columns: valid_ids)"""
        self._tok_event.synchronize()
        return self.logits_host

    def read_logits(self) -> torch.Tensor:
        with torch.cuda.stream(self.stream):
            self.logits_host.copy_(self.logits, non_blocking=True)
            self._tok_event.record(self.stream)
        return self.logits_end()

    def decode_commit(self, tok_start: int, tok_diff: int, tokens: Dict[int, int]):
        """do_sample, second half: graph A2 with `tokens` (every live dialogue's drawn or forced token) as forced tokens"""
        with torch.cuda.stream(self.stream):
            self._set_forced(tokens)
            self._run("A2", self._seq_A2, int(tok_start), int(tok_diff))
            self._tok_event.record(self.stream)

    def speech(self, which: List[int], noise: Optional[Dict[int, torch.Tensor]], sde_noise: Optional[Dict[int, torch.Tensor]] = None,
               frames: Optional[Dict[int, int]] = None):
        """Diffusion sampling for the whole batch (graph H), then the conv tail of the dialogues in `which`, each on its own stream."""
        self.speech_begin(which, noise, sde_noise, frames)
        self.speech_tails(which)

    def _speech_begin_dn(self, which: List[int], frames: Dict[int, int]):
        """device noise: the frame indices of the dialogues in `which` (4 B bytes, the others keep theirs) + the graph H that draws first"""
        with torch.cuda.stream(self.stream):
            prev = self.noise_frame_host[self._frame_k]
            self._frame_k ^= 1
            fh = self.noise_frame_host[self._frame_k]
            fh.copy_(prev)
            for b in which:
                fh[b] = int(frames[b])
            self.noise_frame_dev.copy_(fh, non_blocking=True)
            self._run_H(True)
            self._head_event.record(self.stream)
            if self._timing is not None and self._tcur is not None:
                self._tcur["h1"] = torch.cuda.Event(enable_timing=True)
                self._tcur["h1"].record(self.stream)

    def speech_begin(self, which: List[int], noise: Optional[Dict[int, torch.Tensor]], sde_noise: Optional[Dict[int, torch.Tensor]] = None,
                     frames: Optional[Dict[int, int]] = None):
        """noise upload (the SDE solver: with every step's variance noise [n_steps, latent] per dialogue) + graph H on the main stream.
        frames = {dialogue: frame index}: device noise (set_noise_seeds) - nothing but the indices is uploaded."""
        cfg = self.cfg
        if frames is not None:
            return self._speech_begin_dn(which, frames)
        if self.sde and (sde_noise is None or any(b not in sde_noise or sde_noise[b] is None for b in which)):
            raise L.VVError("the SDE solver needs the per-step variance noise [n_steps, latent] of every diffusing dialogue")
        with torch.cuda.stream(self.stream):
            self._noise_k ^= 1
            nh = self.noise_host[self._noise_k]
            for b in which:
                nh[b].copy_(noise[b].reshape(-1)[: cfg.latent])
            self.noise_dev.copy_(nh, non_blocking=True)
            if self.sde:
                sh = self.sde_noise_host[self._noise_k]
                n_steps = sh.shape[1]
                for b in which:
                    sh[b].copy_(sde_noise[b].reshape(n_steps, -1)[:, : cfg.latent])
                self.sde_noise_dev.copy_(sh, non_blocking=True)
            self._run_H(False)
            self._head_event.record(self.stream)
            if self._timing is not None and self._tcur is not None:
                self._tcur["h1"] = torch.cuda.Event(enable_timing=True)
                self._tcur["h1"].record(self.stream)

    def speech_tails(self, which: List[int]):
        """The conv tails of the dialogues in `which`, enqueued once H HAS FINISHED (late_tails): a lane queue that sits on a cross-stream wait
        while the main queue runs A and H slows every dependent launch there by ~6 us (graph A 1.35 -> 2.28 ms, H 1.72 -> 2.9 ms, measured with
        VV_RB_TIMING=1), so the lanes' queues stay EMPTY until their work can run.  With several row batches in one loop (more than 4 dialogues)
        the caller enqueues every batch's A and H first and the tails afterwards: a batch's tails then overlap the next batch's A and H."""
        late = self.late_tails

        def tail(b):
            e = self.lanes[b]
            torch.cuda.set_device(self.device)
            if late and not self._on_main[b]:
                self._head_event.synchronize()      # the worker itself waits for H: its launch goes out the moment the sampler is done, and needs
            with torch.cuda.stream(e.stream):       # no stream-side wait on the event any more
                e._run("RBconv", self._seq_conv, b, self.uid)
                self._lane_done(b)
                if self._timing is not None and self._tcur is not None:
                    ev = torch.cuda.Event(enable_timing=True)
                    ev.record(e.stream)
                    self._tcur["t"].append(ev)

        self._wait_jobs()       # another row batch's worker may still be feeding (first use: capturing on) one of these streams
        if self.conv_rows is not None:
            return self._speech_tails_rows(which)
        inline = []
        for b in which:
            if self._on_main[b]:
                inline.append(b)
            else:
                if not late:
                    # a cross-stream wait is issued HERE, by the thread that owns the main stream: a wait on an event of a stream that another
                    # thread is capturing (first use of a graph) is a capture-isolation error, and only this thread captures on the main stream
                    self.lanes[b].stream.wait_event(self._head_event)
                _submit(self.lanes[b].stream, tail, b)
        if late and inline:
            self._head_event.synchronize()
        for b in inline:
            e = self.lanes[b]
            if e.use_graphs and ("RBconv", b, self.uid) not in e._graphs:
                _wait_all_jobs()   # first use captures on the main stream: no worker may still be waiting on _head_event (recorded there)
            tail(b)             # this dialogue's tail rides the main stream, behind H

    def embed(self, b: int):
        """next input of dialogue b = embed_tokens[its token], on its stream (after a rollback of that stream, if any)"""
        self._wait_jobs()
        e = self.lanes[b]
        with torch.cuda.stream(e.stream):
            if not self._on_main[b]:
                e.stream.wait_event(self._tok_event)
            e._run("RBembed", self._seq_embed, b, self.uid)
            self._lane_done(b)

    def rollback(self, b: int):
        self._wait_jobs()
        self.lanes[b].rollback_speech_state()
        if self.conv_rows is not None:
            self.conv_rows.rollback(b)      # the mis-speculated frame owes no back; the next front waits for the restore through the lane's event
            self._lane_done(b)

    def reset_speech(self, b: int):
        self._wait_jobs()
        e = self.lanes[b]
        with torch.cuda.stream(e.stream):
            e.reset_speech_caches()
            if self.conv_rows is not None:
                self._lane_done(b)

    def synchronize(self):
        self._wait_jobs()
        for e in self.lanes:
            e.stream.synchronize()
        if self._timing:
            import statistics
            T = [t for t in self._timing if t["h1"] is not None and len(t["t"]) == self.B]
            rows = []
            for i in range(5, len(T) - 1):
                t, nx = T[i], T[i + 1]
                tails = max(t["h1"].elapsed_time(ev) for ev in t["t"])
                rows.append((t["a0"].elapsed_time(t["a1"]), t["a1"].elapsed_time(t["h1"]), tails, t["a0"].elapsed_time(nx["a0"])))
            if rows:
                med = [statistics.median(r[k] for r in rows) for k in range(4)]
                print(f"[rowbatch timing] {len(rows)} steps, medians: A {med[0]:.3f} ms, token copy + noise + H {med[1]:.3f} ms, tails after H {med[2]:.3f} ms, "
                      f"step period {med[3]:.3f} ms (gap {med[3] - med[0] - med[1] - med[2]:.3f})", flush=True)
            self._timing.clear()
