"""Per-GPU VibeVoice engine: device state + the launch sequences of the per-frame loop on the HIP C ABI.

One Engine = one utterance stream on one MI355X (dialogues shard across GPUs, batch 1 per GPU).
Everything numerical goes through libvv_hip.so; torch only owns device memory, the stream and pinned staging.

Per generated token (reference loop: modeling_vibevoice_inference.py:430-673):
  graph A  positive AND negative Qwen2 decode as ONE batch-2 weight pass (the negative row is speculative: it is
           committed only if the chosen token is speech_diffusion, exactly when the reference runs it, :575-587)
           -> 4/5 constrained logits -> argmax -> device-side position bookkeeping
  host     reads the 4-byte token (the only sync of the frame) and runs the reference's token state machine
  graph B  (speech_diffusion) CFG diffusion sampling -> acoustic decode -> semantic encode -> connectors -> next embedding
  graph C  (otherwise) next embedding = embed_tokens[token]
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from .config import VVConfig
from .schedule import DPMSolverMultistepScheduler, timestep_sinusoid
from .weights import DeviceWeights


# HIP streams an Engine gave back, per device.  Streams are recycled, never just dropped: every stream that has run work keeps a hardware
# queue, and on MI355X a process with more than ~5 queues that have ever been active runs concurrent lanes 2-3x slower (measured:
# batch-of-4 generate 69 -> 30 audio-s/s once three more streams had been used, tools/dbg_lanes.py), so the number of streams has to
# stay at the number of engines alive at once.
_IDLE_STREAMS: Dict[str, list] = {}


def check_kv_cache_dtype(kv_cache_dtype: Optional[str], dtype: torch.dtype, head_dim: int) -> bool:
    """Validate the `kv_cache_dtype` option (None / "bf16": no effect at all - the cache stays in the compute dtype, fp32 arithmetic included; "fp8": e4m3 bytes with one power-of-two scale per
    (layer, KV head), decode steps only).  Returns True for the fp8 cache.  Pure host logic: raises ValueError before anything touches a GPU."""
    if kv_cache_dtype is None or kv_cache_dtype == "bf16":
        return False
    if kv_cache_dtype != "fp8":
        raise ValueError(f"kv_cache_dtype={kv_cache_dtype!r}: None, 'bf16' or 'fp8'")
    if dtype != torch.bfloat16:
        raise ValueError(f"kv_cache_dtype='fp8' needs torch_dtype=torch.bfloat16 (the fp8 decode attention widens codes to bf16), not {dtype}")
    if head_dim != 128:
        raise ValueError(f"kv_cache_dtype='fp8' needs head_dim 128 (the grouped-query matrix-core decode kernel), not {head_dim}")
    return True


def write_sampler_row(host: torch.Tensor, b: int, temperature, top_k, top_p) -> tuple:
    """One vv_sampler row {float temperature, int top_k, float top_p} of a pinned fp32 [B, 3] mirror; returns the validated row.  ValueError for a
    row outside the kernels' contract (temperature >= 0 - 0 is greedy -, 0 < top_p <= 1)."""
    t, k, p = float(temperature), int(top_k), float(top_p)
    if not (t >= 0.0 and t < float("inf")) or not (0.0 < p <= 1.0):
        raise ValueError(f"sampler row: temperature={temperature!r} (>= 0, 0 = greedy), top_p={top_p!r} (0 < top_p <= 1)")
    host[b, 0], host[b, 2] = t, p
    host.view(torch.int32)[b, 1] = max(k, 0)
    return (t, max(k, 0), p)


def write_seed_rows(host: torch.Tensor, seeds) -> None:
    """64-bit seeds into a pinned int64 mirror, bit for bit (a seed >= 2^63 is held as its two's complement)"""
    for b, sd in enumerate(seeds):
        v = int(sd) & (2 ** 64 - 1)
        host[b] = v - 2 ** 64 if v >= 2 ** 63 else v


class Engine:
    def __init__(self, cfg: VVConfig, state_dict: Dict[str, torch.Tensor], device="cuda:0", dtype=torch.bfloat16,
                 kv_dtype: Optional[torch.dtype] = None, use_graphs: bool = True, bf16_timestep_quirk: Optional[bool] = None,
                 weight_quant: Optional[str] = None, stream: Optional[torch.cuda.Stream] = None, weights_from: Optional["Engine"] = None,
                 prequant: Optional[dict] = None, kv_cache_dtype: Optional[str] = None, mxfp4_row_batch: bool = False, mxfp4_lean: bool = False,
                 mxfp6_row_batch: bool = False, mxfp6_lean: bool = False):
        self.kv_fp8 = check_kv_cache_dtype(kv_cache_dtype, dtype, cfg.head_dim)
        self.lib = L.load()
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.VVError("the VibeVoice MI355X engine needs a GPU device (there is no CPU path)")
        self.dtype = dtype
        self.kv_dtype = kv_dtype or dtype     # kv_cache_dtype None / "bf16": exactly as without the option; "fp8": the dtype of the prompt's staging cache
        if self.kv_fp8 and self.kv_dtype != torch.bfloat16:
            raise ValueError("kv_cache_dtype='fp8' stages the prompt in a bf16 cache: kv_dtype must be bfloat16")
        self.use_graphs = use_graphs
        self.bf16_t_quirk = (dtype == torch.bfloat16) if bf16_timestep_quirk is None else bf16_timestep_quirk
        torch.cuda.set_device(self.device)
        self._own_stream = stream is None
        if stream is None:                               # `stream`: run on another engine's stream (lanes of a large lock-step batch)
            idle = _IDLE_STREAMS.setdefault(str(self.device), [])
            stream = idle.pop() if idle else torch.cuda.Stream(self.device)
        self.stream = stream
        torch.zeros(1, device=self.device)              # make sure the HIP context exists before the library touches it
        L.check(self.lib.vv_init(), "vv_init")          # one-time kernel attributes, before any graph capture
        self.sync_in()
        with torch.cuda.stream(self.stream):
            # weights_from: another engine of the same model on this device - its weights are used as they are (DeviceWeights.fork), only
            # the streaming state is this engine's own
            # (prequant: the NF4 matrices of a pre-quantized bitsandbytes checkpoint, DeviceWeights)
            if weights_from is not None:
                self.w = weights_from.w.fork()
            else:
                self.w = DeviceWeights(cfg, state_dict, self.device, dtype, quant=weight_quant, prequant=prequant, mxfp4_row_batch=mxfp4_row_batch,
                                       mxfp4_lean=mxfp4_lean, mxfp6_row_batch=mxfp6_row_batch, mxfp6_lean=mxfp6_lean)
            H = cfg.hidden
            f32 = dict(dtype=torch.float32, device=self.device)
            self.x2 = torch.zeros(2, H, **f32)            # input embedding of the step, rows {positive, negative}
            self.hidden2 = torch.zeros(2, H, **f32)       # final-normed hidden states = {condition, negative condition}
            self.lens = torch.zeros(2, dtype=torch.int32, device=self.device)     # positions {positive, negative}
            self.frame_ctr = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.token_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
            self.forced_dev = torch.full((1,), -1, dtype=torch.int32, device=self.device)
            self.noise_dev = torch.zeros(cfg.latent, **f32)
            self.latent = torch.zeros(cfg.latent, **f32)
            self.wav = torch.zeros(cfg.hop, **f32)
            self.sem = torch.zeros(cfg.sem_dim, **f32)
            self.conn_ws = torch.zeros(8 * H, **f32)
            self.logits = torch.zeros(8, **f32)
            self.q_dev = torch.ones(8, **f32)             # device-side do_sample: the step's exponential draws, one per constrained id
            # device-side diffusion noise (vv_noise_normal): the dialogue's 64-bit seed (its bits in an int64) and the index of the frame to draw
            self.noise_seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
            self.noise_frame_dev = torch.zeros(1, dtype=torch.int32, device=self.device)
            # seeded token draws (vv_llm_tail_sample_rows): the dialogue's vv_sampler row {temperature, top_k, top_p} and 64-bit token seed, read
            # on the device - the warpers are no launch argument and the draws are formed there from (seed, position)
            self.sampler_dev = torch.zeros(1, 3, **f32)
            self.tok_seed_dev = torch.zeros(1, dtype=torch.int64, device=self.device)
        self.token_host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.logits_host = torch.zeros(8, dtype=torch.float32).pin_memory()
        self.forced_host = torch.full((1,), -1, dtype=torch.int32).pin_memory()
        self._forced_dev_val = -1                         # what forced_dev holds (see _set_forced)
        self.noise_host = torch.zeros(2, cfg.latent, dtype=torch.float32).pin_memory()   # double-buffered: the host runs a frame ahead
        self._noise_k = 0
        self.noise_seed_host = torch.zeros(1, dtype=torch.int64).pin_memory()            # written once per sequence (set_noise_seed)
        self.noise_frame_host = torch.zeros(2, 1, dtype=torch.int32).pin_memory()        # double-buffered like the noise rows
        self._frame_k = 0
        self.q_host = torch.ones(2, 8, dtype=torch.float32).pin_memory()                 # double-buffered like the noise rows
        self._q_k = 0
        self._sampler, self._sampler_key = None, None     # set_sampler
        self.sampler_host = torch.zeros(1, 3, dtype=torch.float32).pin_memory()          # the pinned mirrors of sampler_dev / tok_seed_dev
        self.sampler_host[0, 2] = 1.0                                                    # greedy: (0, 0, 1)
        self.tok_seed_host = torch.zeros(1, dtype=torch.int64).pin_memory()
        self._sampler_rows = [(0.0, 0, 1.0)]              # set_sampler_row: what sampler_dev holds, for the first token's vv_sample_ids
        self._seeded = False                              # set_token_seeds: this sequence draws its tokens from (token seed, position)
        self._tok_event = torch.cuda.Event()
        # streaming delivery: a frame's 3200 samples go device -> pinned ring asynchronously, an event per
        # slot says when the host may hand them to the AudioStreamer; generate() never blocks the launch queue on a D2H copy
        self._ring = [torch.zeros(cfg.hop, dtype=torch.float32).pin_memory() for _ in range(8)]     # 8 slots: <= 3 chunks wait for delivery, a
        self._ring_ev = [torch.cuda.Event() for _ in range(8)]                                       # mis-speculated frame burns one
        self._ring_n = 0
        self.spec_slot = None
        with torch.cuda.stream(self.stream):
            self._state_snap = torch.empty_like(self.w.state_blob())
        self.scheduler = DPMSolverMultistepScheduler(num_train_timesteps=cfg.ddpm_steps, beta_schedule=cfg.beta_schedule,
                                                     prediction_type=cfg.prediction_type)
        self.n_steps = 0
        self.cfg_scale = 1.3
        self.kv = None
        self._kv_t = None
        self._llm_ws = None
        self._llm_ws_rows = 0
        self.prefill_passes = 0         # vv_llm_prefill_packed calls so far (prefill(packed=True))
        self._graphs: Dict[str, int] = {}
        self._graph_key = None
        self.valid_ids: List[int] = []
        self._w_valid = None
        self._ids_dev = None
        with torch.cuda.stream(self.stream):
            self._alloc_ws()
        self.set_steps(cfg.ddpm_infer)
        self.stream.synchronize()

    # ---------------------------------------------------------------------------------------------------------
    @property
    def sp(self) -> int:
        return self.stream.cuda_stream

    def _ck(self, rc, what):
        L.check(rc, what)

    def sync_in(self):
        """Order the engine stream after whatever the caller enqueued on torch's current stream (inputs, weights)."""
        self.stream.wait_stream(torch.cuda.current_stream(self.device))

    def _alloc_ws(self):
        lib = self.lib
        u8 = dict(dtype=torch.uint8, device=self.device)
        self._dec_ws = torch.empty(lib.vv_convnet_ws_bytes(C.byref(self.w.dec), 1, 1), **u8)
        self._sem_ws = torch.empty(lib.vv_convnet_ws_bytes(C.byref(self.w.sem), self.cfg.hop, 0), **u8)
        self._ensure_llm_ws(2)

    def _ensure_llm_ws(self, rows: int):
        if rows > self._llm_ws_rows:
            n = self.lib.vv_llm_ws_bytes(C.byref(self.w.llm), rows)
            self._llm_ws = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._llm_ws_rows = rows
            self._drop_graphs()

    def _drop_graphs(self):
        for g in self._graphs.values():
            self.lib.vv_graph_destroy(g)
        self._graphs = {}

    # ---------------------------------------------------------------------------------------------------------
    def set_steps(self, n_steps: int):
        """set_ddpm_inference_steps: schedule tables + the step-invariant t_embedder(t_i) table [n, D]."""
        algo = self.scheduler.config["algorithm_type"]
        if n_steps == self.n_steps and algo == getattr(self, "_algo", None):
            return
        self.n_steps, self._algo = n_steps, algo
        self.sde = algo.startswith("sde")            # variance noise per solver step (dpm_solver.py:993-998)
        self.scheduler.set_timesteps(n_steps)
        coefs = (L.DpmCoef * n_steps)()
        for i, c in enumerate(self.scheduler.coefs):
            coefs[i].alpha_s, coefs[i].sigma_s, coefs[i].cx, coefs[i].cd = c["alpha_s"], c["sigma_s"], c["cx"], c["cd"]
            coefs[i].rinv, coefs[i].order, coefs[i].cn = c["rinv"], c["order"], c["cn"]
        self._coefs = coefs
        D = self.cfg.head_hidden
        with torch.cuda.stream(self.stream):
            sin = timestep_sinusoid(self.scheduler.timesteps.numpy(), self.w.t_mlp0.shape[1], bf16_quirk=self.bf16_t_quirk).to(self.device)
            t1 = torch.empty(n_steps, D, dtype=torch.float32, device=self.device)
            self.temb = torch.empty(n_steps, D, dtype=torch.float32, device=self.device)
            self.linear(sin, self.w.t_mlp0, t1)
            self.linear(t1, self.w.t_mlp2, self.temb, pro=L.PRO_SILU)
            self._head_ws = torch.empty(self.lib.vv_head_ws_bytes(C.byref(self.w.head), n_steps), dtype=torch.uint8, device=self.device)
            self.sde_noise_dev = torch.zeros(n_steps, self.cfg.latent, dtype=torch.float32, device=self.device)
        self.sde_noise_host = torch.zeros(2, n_steps, self.cfg.latent, dtype=torch.float32).pin_memory()
        self._drop_graphs()

    def linear(self, x, w, out, pro=L.PRO_NONE, bias=None):
        """thin vv_linear wrapper for [m,k] x [n,k]^T (host-side table building and tests)."""
        a = L.LinArgs()
        a.x, a.ldx, a.m = x.data_ptr(), x.stride(0), x.shape[0]
        a.pro = pro
        a.w, a.n, a.k = w.data_ptr(), w.shape[0], w.shape[1]
        a.wdt = L.VV_F32 if w.dtype == torch.float32 else L.VV_BF16
        a.bias = L.ptr(bias)
        a.out, a.ldo = out.data_ptr(), out.stride(0)
        self._ck(self.lib.vv_linear(C.byref(a), self.sp), "vv_linear")

    # ---------------------------------------------------------------------------------------------------------
    def begin_sequence(self, s_max: int, valid_ids: List[int]):
        """Fresh utterance: KV cache sized for s_max tokens, conv states zeroed, constrained-vocabulary rows gathered."""
        cfg = self.cfg
        with torch.cuda.stream(self.stream):
            self._ensure_kv(s_max)
            ids = sorted(set(int(i) for i in valid_ids))
            if ids != self.valid_ids:
                self.valid_ids = ids
                arr = (C.c_int * len(ids))(*ids)
                self._w_valid = torch.empty(len(ids), cfg.hidden, dtype=self.dtype, device=self.device)
                self._ck(self.lib.vv_gather_rows(self.w.lm_head.data_ptr(), self.w.wdt, cfg.hidden, arr, len(ids),
                                                 self._w_valid.data_ptr(), self.sp), "vv_gather_rows")
                self._ids_dev = torch.tensor(ids, dtype=torch.int32, device=self.device)
                self._drop_graphs()
            self.lens.zero_()
            self.frame_ctr.zero_()
            self.reset_speech_caches()
        self._seeded = False

    def _ensure_kv(self, s_max: int):
        """The KV cache (rows {positive, negative}) with room for s_max tokens; call it under `torch.cuda.stream(self.stream)`."""
        cfg = self.cfg
        s_max = (int(s_max) + 63) // 64 * 64
        if self.kv is None or self.kv.s_max < s_max:
            shape = (cfg.layers, 2, cfg.kv_heads, s_max, cfg.head_dim)
            cdt = torch.uint8 if self.kv_fp8 else self.kv_dtype        # fp8: e4m3fn codes, one byte per element, same shapes
            self._kv_t = (torch.zeros(shape, dtype=cdt, device=self.device),
                          torch.zeros(shape, dtype=cdt, device=self.device))
            kv = L.KV()
            kv.k, kv.v = self._kv_t[0].data_ptr(), self._kv_t[1].data_ptr()
            if self.kv_fp8:
                self._kv_vt = torch.empty((cfg.layers, 2, cfg.kv_heads, s_max // 32, cfg.head_dim, 32), dtype=cdt, device=self.device)
                self._kv_scale = torch.ones(2, cfg.layers, cfg.kv_heads, dtype=torch.float32, device=self.device)     # {k, v}: set by prefill
                kv.vt = self._kv_vt.data_ptr()
                kv.kscale, kv.vscale = self._kv_scale[0].data_ptr(), self._kv_scale[1].data_ptr()
            elif self.kv_dtype == torch.bfloat16 and cfg.head_dim == 128:
                # transposed value cache in 32-key tiles [.., s_max / 32, head_dim, 32] for the matrix-core attention kernels (kept in step
                # with v by vv_rope_store for prompt rows and by vv_attn_decode for decode steps)
                self._kv_vt = torch.empty((cfg.layers, 2, cfg.kv_heads, s_max // 32, cfg.head_dim, 32), dtype=self.kv_dtype, device=self.device)
                kv.vt = self._kv_vt.data_ptr()
            kv.kvdt = L.VV_FP8 if self.kv_fp8 else (L.VV_F32 if self.kv_dtype == torch.float32 else L.VV_BF16)
            kv.layers, kv.rows, kv.kv_heads, kv.s_max, kv.head_dim = cfg.layers, 2, cfg.kv_heads, s_max, cfg.head_dim
            self.kv = kv
            self._drop_graphs()

    def reset_speech_caches(self):
        """acoustic_cache.set_to_zero / semantic_cache.set_to_zero (modeling_vibevoice_inference.py:540-544)."""
        self._ck(self.lib.vv_convnet_reset(C.byref(self.w.dec), self.sp), "vv_convnet_reset")
        self._ck(self.lib.vv_convnet_reset(C.byref(self.w.sem), self.sp), "vv_convnet_reset")

    # ---------------------------------------------------------------------------------------------------------
    # component launch sequences (all asynchronous on self.stream)
    # ---------------------------------------------------------------------------------------------------------
    def llm_forward(self, x: torch.Tensor, lens: torch.Tensor, cache_rows: Optional[torch.Tensor], out: torch.Tensor, kv=None):
        R = x.shape[0]
        self._ensure_llm_ws(R)
        self._ck(self.lib.vv_llm_forward(C.byref(self.w.llm), C.byref(kv or self.kv), x.data_ptr(), x.stride(0), R, lens.data_ptr(),
                                         L.ptr(cache_rows), out.data_ptr(), out.stride(0), self._llm_ws.data_ptr(), self.sp),
                 "vv_llm_forward")

    def llm_prefill_packed(self, x: torch.Tensor, lens: torch.Tensor, cache_rows: torch.Tensor, sel: torch.Tensor, out: torch.Tensor, kv=None):
        """vv_llm_prefill_packed: the prefill pass whose matrix-core linears carry VV_LIN_PACKED; out [len(sel), H] = the selected rows' states"""
        R = x.shape[0]
        self._ensure_llm_ws(R)
        self._ck(self.lib.vv_llm_prefill_packed(C.byref(self.w.llm), C.byref(kv or self.kv), x.data_ptr(), x.stride(0), R, lens.data_ptr(),
                                                cache_rows.data_ptr(), sel.data_ptr(), sel.shape[0], out.data_ptr(), out.stride(0),
                                                self._llm_ws.data_ptr(), self.sp), "vv_llm_prefill_packed")

    def prefill(self, embeds: torch.Tensor, row: int = 0, pos0: int = 0, chunk: int = 1024, neg_embed: Optional[torch.Tensor] = None,
                prefix=None, keep_staging: bool = False, packed: bool = False):
        """Prompt prefill on cache row `row`: embeds [L0, H] fp32 -> self.hidden2[row] = last hidden state; lens[row] = pos0+L0.
        Prompts longer than `chunk` rows run as ceil(L0 / chunk) EQUAL chunks (rounded up to 32 rows): a short trailing chunk would stream
        every weight matrix once more for a handful of rows (1 040 tokens as 1 024 + 16 cost 18.5 ms, as 2 x 520 they cost 12).
        neg_embed [1, H]: the negative branch's one-token prompt (a single speech_start, modeling_vibevoice_inference.py:377-381) rides along as
        one more row of the last chunk - cache row 1, position 0 - instead of a weight pass of its own (1.1 ms of the first chunk's latency);
        hidden2[1] then holds its state and the CALLER sets lens[1] = 1 if the branch is in use (`commit_negative_prompt`).
        prefix (a VoicePrefix, voice_prefix.py): its P slots are restored into slots [0, P) of the row with one vv_kv_copy and `embeds` - the rows
        after the prefix only - are prefilled at position P (pos0 must be 0: the prefix implies it).  On an fp8 KV cache the restore goes into the
        staging cache, sized for P + L0, and the scales are derived from all P + L0 slots, as without a prefix.
        keep_staging (fp8 KV cache): skip the conversion and return the staging cache (vv_kv, its tensors) - how save_prefix gets at the prompt's
        bf16 K / V; the byte cache is left alone and the engine is not ready to decode.
        packed (packed_prefill): every chunk runs through vv_llm_prefill_packed - one segment plus the negative row - so its GEMMs may take the
        packed-prefill tile kernel, and only the rows whose state is kept are final-normed; `chunk` is then the rows per pass."""
        L0 = embeds.shape[0]
        P = 0
        if prefix is not None:
            if pos0 != 0:
                raise L.VVError("prefill: a prefix fixes the position of the rows after it (pos0 must be 0)")
            P = int(prefix.P)
        kv, stage = None, None
        if self.kv_fp8:
            # fp8 KV cache: the prompt runs exactly as on a bf16 cache, on a bf16 staging cache sized to the prompt (rows 0 and 1: the negative
            # branch's one-token prompt is a row of this prefill); its rows are then converted into the byte cache and the staging cache freed
            if pos0 != 0 or row != 0:
                raise L.VVError("kv_cache_dtype='fp8': the prompt is prefilled once, at position 0 of cache row 0 (prompt attention has no fp8-KV form)")
            with torch.cuda.stream(self.stream):     # allocated, zeroed, used and freed on the engine's stream: the allocator reuses it in that stream's order
                kv, stage = self._staging_kv(P + L0)
        elif keep_staging:
            raise L.VVError("prefill(keep_staging=True) is for an fp8 KV cache (any other cache holds the prompt's K / V itself)")
        pos0 += P
        n_chunks = max(1, -(-L0 // max(1, chunk)))
        size = -(-L0 // n_chunks)
        size = min(chunk, (size + 31) // 32 * 32) if n_chunks > 1 else L0
        with torch.cuda.stream(self.stream):
            if prefix is not None:
                self._ck(self.lib.vv_kv_copy(C.byref(prefix.kv), 0, C.byref(kv or self.kv), row, P, self.sp), "vv_kv_copy")
            for c0 in range(0, L0, size):
                c1 = min(L0, c0 + size)
                n = c1 - c0
                last = c1 == L0 and neg_embed is not None
                lens = torch.arange(pos0 + c0, pos0 + c1 + (1 if last else 0), dtype=torch.int32, device=self.device)
                rows = torch.full((n + (1 if last else 0),), row, dtype=torch.int32, device=self.device)
                x = embeds[c0:c1].contiguous()
                if last:
                    lens[-1] = 0
                    rows[-1] = 1
                    x = torch.cat([x, neg_embed.to(x.dtype).reshape(1, -1)])
                if packed:
                    sel = torch.arange(n - 1, n + (1 if last else 0), dtype=torch.int32, device=self.device)      # the segment's last row (, the negative row)
                    out = torch.empty(sel.shape[0], self.cfg.hidden, dtype=torch.float32, device=self.device)
                    self.llm_prefill_packed(x, lens, rows, sel, out, kv=kv)
                    self.prefill_passes += 1
                    continue
                out = torch.empty(x.shape[0], self.cfg.hidden, dtype=torch.float32, device=self.device)
                self.llm_forward(x, lens, rows, out, kv=kv)
            if stage is not None and not keep_staging:
                # row 0 sets the scales of every (layer, KV head) from the prompt's K / V absmax; row 1 (the negative prompt) reuses them
                self._ck(self.lib.vv_kv_quantize(C.byref(kv), C.byref(self.kv), 0, 0, pos0 + L0, L.KVQ_DERIVE_SCALES, self.sp), "vv_kv_quantize")
                self._ck(self.lib.vv_kv_quantize(C.byref(kv), C.byref(self.kv), 1, 1, 1 if neg_embed is not None else 0, 0, self.sp), "vv_kv_quantize")
                del stage, kv         # back to the pool of the engine's stream, on which it was allocated (see above)
            if neg_embed is not None:
                self.hidden2[row].copy_(out[-2])
                self.hidden2[1].copy_(out[-1])
            else:
                self.hidden2[row].copy_(out[-1])
            self.lens[row] = pos0 + L0
        if keep_staging:
            return kv, stage

    def save_prefix(self, ids: torch.Tensor, row: int = 0, kv=None):
        """The first P = len(ids) slots of cache row `row` (of `kv`, default the engine's cache; an fp8 engine passes the staging cache that
        prefill(keep_staging=True) returned) as a freshly allocated VoicePrefix: one vv_kv_copy.  Synchronises: the store is complete and
        read-only when this returns."""
        from . import voice_prefix as VP
        cfg = self.cfg
        src = kv or self.kv
        if src is None or src.kvdt == L.VV_FP8:
            raise L.VVError("save_prefix: no bf16 / fp32 cache to read (an fp8 KV cache is saved from its staging cache)")
        ids = torch.as_tensor(ids).reshape(-1).cpu().long().clone()
        P = int(ids.numel())
        with torch.cuda.stream(self.stream):
            shape = VP.store_shape(cfg.layers, cfg.kv_heads, cfg.head_dim, P)
            k = torch.zeros(shape, dtype=self.kv_dtype, device=self.device)
            v = torch.zeros(shape, dtype=self.kv_dtype, device=self.device)
            skv = VP.describe(k, v)
            self._ck(self.lib.vv_kv_copy(C.byref(src), row, C.byref(skv), 0, P, self.sp), "vv_kv_copy")
        self.stream.synchronize()
        return VP.VoicePrefix(ids=ids, P=P, k=k, v=v, kv=skv, nbytes=k.numel() * k.element_size() + v.numel() * v.element_size())

    def _staging_kv(self, n_tokens: int):
        """bf16 cache for a prompt of n_tokens (rounded up to the caches' 64-slot granule), rows {positive, negative}: (vv_kv, its tensors).
        Call it under `torch.cuda.stream(self.stream)`: the tensors must belong to the stream that uses them."""
        cfg = self.cfg
        s_max = max(64, (int(n_tokens) + 63) // 64 * 64)
        shape = (cfg.layers, 2, cfg.kv_heads, s_max, cfg.head_dim)
        t = (torch.zeros(shape, dtype=torch.bfloat16, device=self.device), torch.zeros(shape, dtype=torch.bfloat16, device=self.device),
             torch.empty((cfg.layers, 2, cfg.kv_heads, s_max // 32, cfg.head_dim, 32), dtype=torch.bfloat16, device=self.device))
        kv = L.KV()
        kv.k, kv.v, kv.vt = t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr()
        kv.kvdt = L.VV_BF16
        kv.layers, kv.rows, kv.kv_heads, kv.s_max, kv.head_dim = cfg.layers, 2, cfg.kv_heads, s_max, cfg.head_dim
        return kv, t

    def commit_negative_prompt(self):
        """the negative branch consumed its one-token prompt (see prefill, neg_embed)"""
        with torch.cuda.stream(self.stream):
            self.lens[1] = 1

    def _logits(self):
        a = L.LinArgs()
        nv = len(self.valid_ids)
        a.x, a.ldx, a.m = self.hidden2.data_ptr(), self.cfg.hidden, 1
        a.w, a.n, a.k, a.wdt = self._w_valid.data_ptr(), nv, self.cfg.hidden, self.w.wdt
        a.out, a.ldo = self.logits.data_ptr(), nv
        self._ck(self.lib.vv_linear(C.byref(a), self.sp), "lm_head")

    def _select_token(self):
        self._logits()
        self._pick()

    def _pick(self):
        nv = len(self.valid_ids)
        self._ck(self.lib.vv_argmax_ids(self.logits.data_ptr(), nv, self._ids_dev.data_ptr(), self.token_dev.data_ptr(),
                                        self.forced_dev.data_ptr(), self.sp), "vv_argmax_ids")

    def _seq_A(self, tok_start, tok_diff):
        """batch-2 decode step + token selection + device-side position bookkeeping: the Qwen2 stack leaves its un-normalised last
        hidden rows at the start of the workspace, vv_llm_tail does final norm + constrained logits + argmax / forced token +
        position update in ONE launch."""
        nv = len(self.valid_ids)
        self._ck(self.lib.vv_llm_forward(C.byref(self.w.llm), C.byref(self.kv), self.x2.data_ptr(), self.cfg.hidden, 2,
                                         self.lens.data_ptr(), None, None, 0, self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._ck(self.lib.vv_llm_tail(C.byref(self.w.llm), self._llm_ws.data_ptr(), self.cfg.hidden, 2, self.hidden2.data_ptr(), self.cfg.hidden,
                                      self._w_valid.data_ptr(), nv, self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(),
                                      self.forced_dev.data_ptr(), self.lens.data_ptr(), tok_start, tok_diff, self.frame_ctr.data_ptr(), self.sp),
                 "vv_llm_tail")

    def _seq_AS(self, tok_start, tok_diff, temperature, top_k, top_p):
        """_seq_A with the sampling tail: the token is drawn on the device from the warped constrained logits and the host's exponential
        draws in q_dev (vv_llm_tail_sample).  The warpers are kernel arguments, i.e. part of the captured graph: they are part of its key
        (_run), a call with other warpers captures a graph of its own."""
        nv = len(self.valid_ids)
        smp = L.Sampler(temperature, top_k, top_p)
        self._ck(self.lib.vv_llm_forward(C.byref(self.w.llm), C.byref(self.kv), self.x2.data_ptr(), self.cfg.hidden, 2,
                                         self.lens.data_ptr(), None, None, 0, self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._ck(self.lib.vv_llm_tail_sample(C.byref(self.w.llm), self._llm_ws.data_ptr(), self.cfg.hidden, 2, self.hidden2.data_ptr(), self.cfg.hidden,
                                             self._w_valid.data_ptr(), nv, self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(),
                                             self.forced_dev.data_ptr(), self.lens.data_ptr(), tok_start, tok_diff, self.frame_ctr.data_ptr(),
                                             C.byref(smp), self.q_dev.data_ptr(), self.sp), "vv_llm_tail_sample")

    def _seq_Ar(self, tok_start, tok_diff):
        """_seq_A with the seeded tail (vv_llm_tail_sample_rows): the warpers and the token seed are read from sampler_dev / tok_seed_dev and
        the draws formed in the kernel from (seed, lens[0]), so the graph's key holds no warpers and nothing is uploaded per step; a greedy
        row (temperature 0) takes the argmax in the same graph."""
        nv = len(self.valid_ids)
        self._ck(self.lib.vv_llm_forward(C.byref(self.w.llm), C.byref(self.kv), self.x2.data_ptr(), self.cfg.hidden, 2,
                                         self.lens.data_ptr(), None, None, 0, self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._ck(self.lib.vv_llm_tail_sample_rows(C.byref(self.w.llm), self._llm_ws.data_ptr(), self.cfg.hidden, 2, self.hidden2.data_ptr(), self.cfg.hidden,
                                                  self._w_valid.data_ptr(), nv, self._ids_dev.data_ptr(), self.logits.data_ptr(), self.token_dev.data_ptr(),
                                                  self.forced_dev.data_ptr(), self.lens.data_ptr(), tok_start, tok_diff, self.frame_ctr.data_ptr(),
                                                  self.sampler_dev.data_ptr(), self.tok_seed_dev.data_ptr(), self.sp), "vv_llm_tail_sample_rows")

    def _seq_A1(self):
        self._ck(self.lib.vv_llm_forward(C.byref(self.w.llm), C.byref(self.kv), self.x2.data_ptr(), self.cfg.hidden, 2,
                                         self.lens.data_ptr(), None, self.hidden2.data_ptr(), self.cfg.hidden,
                                         self._llm_ws.data_ptr(), self.sp), "vv_llm_forward")
        self._logits()

    def _seq_A2(self, tok_start, tok_diff):
        self._pick()
        self._ck(self.lib.vv_advance_lens(self.lens.data_ptr(), self.token_dev.data_ptr(), tok_start, tok_diff,
                                          self.frame_ctr.data_ptr(), self.sp), "vv_advance_lens")

    def _seq_noise(self):
        """device noise: the frame's initial latent - and the SDE solver's per-step variance noise - drawn into noise_dev / sde_noise_dev from
        (noise_seed_dev, noise_frame_dev) by one launch at the head of the frame's graph"""
        cfg = self.cfg
        self._ck(self.lib.vv_noise_normal(self.noise_dev.data_ptr(), cfg.latent, self.sde_noise_dev.data_ptr() if self.sde else None,
                                          self.n_steps * cfg.latent, 1, cfg.latent, self.n_steps if self.sde else 0, self.noise_seed_dev.data_ptr(),
                                          self.noise_frame_dev.data_ptr(), self.sp), "vv_noise_normal")

    def _seq_B(self, cfg_scale, dn=None):
        """speech_diffusion tail: sample latent, decode audio, re-encode semantics, build the next embedding.  dn == "dn": the noise is drawn
        on the device first (_seq_noise); the marker is part of the graph's key, so ("B", cfg_scale) stays the graph it was."""
        lib, w, cfg = self.lib, self.w, self.cfg
        if dn:
            self._seq_noise()
        # snapshot of the streaming state (one ~1.4 MB copy): lets a frame that was launched speculatively be rolled back
        blob = w.state_blob()
        self._ck(lib.vv_copy_rows(blob.data_ptr(), blob.numel(), self._state_snap.data_ptr(), blob.numel(), 1, blob.numel(), self.sp), "snapshot")
        self._ck(lib.vv_head_sample(C.byref(w.head), self.hidden2.data_ptr(), cfg.hidden, self.noise_dev.data_ptr(),
                                    self.temb.data_ptr(), self._coefs, self.n_steps, cfg_scale, self.latent.data_ptr(),
                                    self._head_ws.data_ptr(), self.sde_noise_dev.data_ptr() if self.sde else None, self.sp), "vv_head_sample")
        self._ck(lib.vv_decoder_forward(C.byref(w.dec), self.latent.data_ptr(), 1, 1.0 / w.speech_scale, -w.speech_bias,
                                        self.wav.data_ptr(), self._dec_ws.data_ptr(), self.sp), "vv_decoder_forward")
        self._ck(lib.vv_encoder_forward(C.byref(w.sem), self.wav.data_ptr(), cfg.hop, self.sem.data_ptr(),
                                        self._sem_ws.data_ptr(), self.sp), "vv_encoder_forward")
        self._ck(lib.vv_connector_pair(C.byref(w.ac_conn), C.byref(w.sem_conn), self.latent.data_ptr(), self.sem.data_ptr(), self.x2.data_ptr(), cfg.hidden, 2,
                                       self.conn_ws.data_ptr(), self.sp), "connectors")

    def _seq_B1(self, cfg_scale, dn=None):
        """first half of _seq_B, up to the frame's audio (streaming delivery: the chunk's D2H copy goes out between the halves)"""
        lib, w, cfg = self.lib, self.w, self.cfg
        if dn:
            self._seq_noise()
        blob = w.state_blob()
        self._ck(lib.vv_copy_rows(blob.data_ptr(), blob.numel(), self._state_snap.data_ptr(), blob.numel(), 1, blob.numel(), self.sp), "snapshot")
        self._ck(lib.vv_head_sample(C.byref(w.head), self.hidden2.data_ptr(), cfg.hidden, self.noise_dev.data_ptr(),
                                    self.temb.data_ptr(), self._coefs, self.n_steps, cfg_scale, self.latent.data_ptr(),
                                    self._head_ws.data_ptr(), self.sde_noise_dev.data_ptr() if self.sde else None, self.sp), "vv_head_sample")
        self._ck(lib.vv_decoder_forward(C.byref(w.dec), self.latent.data_ptr(), 1, 1.0 / w.speech_scale, -w.speech_bias,
                                        self.wav.data_ptr(), self._dec_ws.data_ptr(), self.sp), "vv_decoder_forward")

    def _seq_B2(self):
        """second half of _seq_B: semantic re-encode of the frame and the next step's input embedding"""
        lib, w, cfg = self.lib, self.w, self.cfg
        self._ck(lib.vv_encoder_forward(C.byref(w.sem), self.wav.data_ptr(), cfg.hop, self.sem.data_ptr(),
                                        self._sem_ws.data_ptr(), self.sp), "vv_encoder_forward")
        self._ck(lib.vv_connector_pair(C.byref(w.ac_conn), C.byref(w.sem_conn), self.latent.data_ptr(), self.sem.data_ptr(), self.x2.data_ptr(), cfg.hidden, 2,
                                       self.conn_ws.data_ptr(), self.sp), "connectors")

    def _speech(self, cfg_scale: float, stage: bool, dn: bool = False) -> Optional[int]:
        """Phase B on the current stream.  stage: a consumer is waiting for the audio (AudioStreamer) - the frame runs as two graphs and the
        chunk's device -> pinned copy is enqueued BETWEEN them, as soon as the acoustic decoder has produced it: the chunk reaches the host
        ~0.5 ms earlier than behind the semantic encoder and the connectors (which only the NEXT step needs).  Returns the ring slot."""
        key = (cfg_scale, "dn") if dn else (cfg_scale,)
        if not stage:
            self._run("B", self._seq_B, *key)
            return None
        self._run("B1", self._seq_B1, *key)
        k = self._ring_n % len(self._ring)
        self._ring_n += 1
        self._ring[k].copy_(self.wav, non_blocking=True)
        self._ring_ev[k].record(self.stream)
        self._run("B2", self._seq_B2)
        return k

    def _seq_C(self):
        """next embedding = embed_tokens[token] for both rows (modeling_vibevoice_inference.py:567)."""
        cfg = self.cfg
        self._ck(self.lib.vv_embed_row(self.w.embed.data_ptr(), self.w.wdt, cfg.hidden, self.token_dev.data_ptr(), self.x2.data_ptr(), self.sp), "embed")
        self._ck(self.lib.vv_copy_rows(self.x2.data_ptr(), 0, self.x2.data_ptr() + 4 * cfg.hidden, cfg.hidden, 1, cfg.hidden, self.sp), "copy")

    def _run(self, name: str, fn, *args):
        """Run a launch sequence, through a cached hipGraph when enabled."""
        if not self.use_graphs:
            fn(*args)
            return
        key = (name,) + tuple(args)
        g = self._graphs.get(key)
        if g is None:
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

    # ---------------------------------------------------------------------------------------------------------
    # the three per-token phases used by generate()
    # ---------------------------------------------------------------------------------------------------------
    def _set_forced(self, forced: Optional[int]):
        """Device-side forced token (-1: none).  Uploaded only when it changes: in the steady state of a dialogue (greedy decoding, or a forced
        schedule of speech_diffusion frames) the value repeats and the 4-byte H2D blit (~5 us on the frame's critical path) is skipped.  The
        pinned word is rewritten only after the previous step's token has been awaited, i.e. after any earlier copy from it has executed."""
        v = -1 if forced is None else int(forced)
        if v == self._forced_dev_val:
            return
        self.forced_host[0] = v
        self.forced_dev.copy_(self.forced_host, non_blocking=True)
        self._forced_dev_val = v

    def set_sampler(self, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0):
        """The warpers of the device-side token draw (steps given `q`), fixed per generate() call."""
        self._sampler_key = (float(temperature), int(top_k), float(top_p))
        self._sampler = L.Sampler(*self._sampler_key)

    def set_sampler_row(self, b: int, temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0):
        """Seeded token draws: the dialogue's own warpers, kept on the device (b is 0: an Engine runs one dialogue).  Greedy = (0, 0, 1).  The
        row is validated here - the kernel only promises memory safety for anything else."""
        self._sampler_rows[b] = write_sampler_row(self.sampler_host, b, temperature, top_k, top_p)
        with torch.cuda.stream(self.stream):
            self.sampler_dev.copy_(self.sampler_host, non_blocking=True)

    def set_token_seeds(self, seeds):
        """Seeded token draws: the 64-bit token seed of the dialogue this engine runs next, once per sequence (after begin_sequence).  Every
        step then draws its token on the device from (seed, position, its own logits): graph "Ar", no q, no upload."""
        write_seed_rows(self.tok_seed_host, seeds)
        with torch.cuda.stream(self.stream):
            self.tok_seed_dev.copy_(self.tok_seed_host, non_blocking=True)
        self._seeded = True

    def _upload_q(self, q: torch.Tensor):
        """The step's exponential draws (CPU fp32 [nv]): pinned staging row + async copy on the engine stream, like _upload_noise."""
        if self._sampler is None:
            raise L.VVError("device-side sampling needs set_sampler() first")
        self._q_k ^= 1
        qh = self.q_host[self._q_k]
        qh[: q.numel()].copy_(q.reshape(-1))
        self.q_dev.copy_(qh, non_blocking=True)

    def _phase_A(self, tok_start: int, tok_diff: int, q: Optional[torch.Tensor]):
        """graph A; with draws `q` its sampling variant; after set_token_seeds the seeded one, whose key holds no warpers"""
        if self._seeded:
            self._run("Ar", self._seq_Ar, int(tok_start), int(tok_diff))
        elif q is None:
            self._run("A", self._seq_A, int(tok_start), int(tok_diff))
        else:
            self._upload_q(q)
            self._run("AS", self._seq_AS, int(tok_start), int(tok_diff), *self._sampler_key)

    def _host_logits(self) -> torch.Tensor:
        with torch.cuda.stream(self.stream):
            self.logits_host.copy_(self.logits, non_blocking=True)
        self.stream.synchronize()
        return self.logits_host[: len(self.valid_ids)].clone()

    def step_decode(self, tok_start: int, tok_diff: int, forced: Optional[int] = None, sample_fn=None, on_enqueued=None, q=None) -> int:
        """Phase A + the frame's only host sync: returns the chosen token.  With `sample_fn(logits, ids) -> token` (do_sample, host sampler)
        the constrained logits are read back first and the sampled token is fed to the device-side bookkeeping.  With `q` (do_sample,
        device sampler: the step's exponential draws [nv], set_sampler) the token is drawn inside graph A: one graph, one 4-byte read-back."""
        if sample_fn is not None and forced is None:
            with torch.cuda.stream(self.stream):
                self._run("A1", self._seq_A1)
            tok = int(sample_fn(self._host_logits(), self.valid_ids))
            with torch.cuda.stream(self.stream):
                self._set_forced(tok)
                self._run("A2", self._seq_A2, int(tok_start), int(tok_diff))
            self.stream.synchronize()
            return tok
        with torch.cuda.stream(self.stream):
            self._set_forced(forced)
            self._phase_A(tok_start, tok_diff, q)
            self.token_host.copy_(self.token_dev, non_blocking=True)
        if on_enqueued is not None:
            on_enqueued()
        self.stream.synchronize()
        return int(self.token_host[0])

    def first_token(self, tok_start: int, tok_diff: int, forced: Optional[int] = None, sample_fn=None, q=None) -> int:
        """Token selection right after prefill (hidden2[0] already holds the last prompt state); `q`: drawn on the device (step_decode).
        After set_token_seeds the draws come from vv_token_draws at the last prompt position (lens[0] - 1) and the choice is the row's own
        sampler's (vv_sample_ids), or the argmax for a greedy row."""
        if self._seeded and forced is None:
            nv = len(self.valid_ids)
            with torch.cuda.stream(self.stream):
                self._set_forced(None)
                self._logits()
                if self._sampler_rows[0][0] > 0:
                    self._ck(self.lib.vv_token_draws(self.q_dev.data_ptr(), 8, 1, nv, self.tok_seed_dev.data_ptr(), self.lens.data_ptr(), 2, -1, self.sp),
                             "vv_token_draws")
                    self._ck(self.lib.vv_sample_ids(self.logits.data_ptr(), nv, self._ids_dev.data_ptr(), C.byref(L.Sampler(*self._sampler_rows[0])),
                                                    self.q_dev.data_ptr(), self.token_dev.data_ptr(), self.forced_dev.data_ptr(), self.sp), "vv_sample_ids")
                else:
                    self._pick()
                self.token_host.copy_(self.token_dev, non_blocking=True)
            self.stream.synchronize()
            return int(self.token_host[0])
        if q is not None and forced is None:
            with torch.cuda.stream(self.stream):
                self._set_forced(None)
                self._upload_q(q)
                self._logits()
                self._ck(self.lib.vv_sample_ids(self.logits.data_ptr(), len(self.valid_ids), self._ids_dev.data_ptr(), C.byref(self._sampler),
                                                self.q_dev.data_ptr(), self.token_dev.data_ptr(), self.forced_dev.data_ptr(), self.sp), "vv_sample_ids")
                self.token_host.copy_(self.token_dev, non_blocking=True)
            self.stream.synchronize()
            return int(self.token_host[0])
        if sample_fn is not None and forced is None:
            with torch.cuda.stream(self.stream):
                self._logits()
            forced = int(sample_fn(self._host_logits(), self.valid_ids))
        with torch.cuda.stream(self.stream):
            self._set_forced(forced)
            self._select_token()
            self.token_host.copy_(self.token_dev, non_blocking=True)
        self.stream.synchronize()
        return int(self.token_host[0])

    def _upload_noise(self, noise: torch.Tensor, sde_noise: Optional[torch.Tensor]):
        """Host staging (double-buffered pinned rows: the host runs up to a frame ahead) + async copies on the engine stream."""
        self._noise_k ^= 1
        nh = self.noise_host[self._noise_k]
        nh.copy_(noise.reshape(-1)[: self.cfg.latent])
        self.noise_dev.copy_(nh, non_blocking=True)
        if self.sde:
            if sde_noise is None:
                raise L.VVError("the SDE solver needs the per-step variance noise [n_steps, latent]")
            sh = self.sde_noise_host[self._noise_k]
            sh.copy_(sde_noise.reshape(self.n_steps, -1)[:, : self.cfg.latent])
            self.sde_noise_dev.copy_(sh, non_blocking=True)

    def set_noise_seed(self, seed: int):
        """Device noise: the 64-bit seed of the dialogue this engine runs next, once per sequence (after begin_sequence).  Every frame given a
        `frame` index then draws its noise on the device as a function of (seed, frame) alone."""
        s = int(seed) & (2 ** 64 - 1)
        self.noise_seed_host[0] = s - 2 ** 64 if s >= 2 ** 63 else s      # the seed's 64 bits, held in an int64
        with torch.cuda.stream(self.stream):
            self.noise_seed_dev.copy_(self.noise_seed_host, non_blocking=True)

    def _upload_frame(self, frame: int):
        """Device noise: the index of the frame about to be enqueued - a 4-byte async copy in place of the noise rows (double-buffered pinned
        word: the host runs up to a frame ahead)"""
        self._frame_k ^= 1
        fh = self.noise_frame_host[self._frame_k]
        fh[0] = int(frame)
        self.noise_frame_dev.copy_(fh, non_blocking=True)

    def _noise_in(self, noise, sde_noise, frame) -> bool:
        """what a frame's noise comes from: its index (device noise, True) or the host's rows (False)"""
        if frame is not None:
            self._upload_frame(frame)
            return True
        self._upload_noise(noise, sde_noise)
        return False

    def step_speech(self, noise: Optional[torch.Tensor], sde_noise: Optional[torch.Tensor] = None, stage: bool = False, frame: Optional[int] = None) -> Optional[int]:
        """Phase B.  `noise` is the CPU fp32 [latent] row the reference would have drawn (modeling_vibevoice_inference.py:699),
        `sde_noise` [n_steps, latent] the variance noise of the SDE solver's steps (dpm_solver.py:993-998), if that solver is set.
        stage: also enqueue the chunk's copy to the pinned ring as soon as the decoder is done (see _speech); returns the slot.
        frame: device noise (set_noise_seed) - the frame's index is uploaded instead and the rows are drawn inside the graph."""
        with torch.cuda.stream(self.stream):
            dn = self._noise_in(noise, sde_noise, frame)
            return self._speech(float(self.cfg_scale), stage, dn)

    def step_decode_speculative(self, tok_start: int, tok_diff: int, forced: Optional[int], noise: Optional[torch.Tensor],
                                sde_noise: Optional[torch.Tensor] = None, on_enqueued=None, stage: bool = False, q=None, frame: Optional[int] = None) -> int:
        """Phase A, then phase B enqueued right behind it ON THE ASSUMPTION that the token is speech_diffusion (the steady state
        of a dialogue), then one host wait on the token alone.  The GPU therefore never idles between A and B while the host
        wakes up and decides; if the token turns out to be something else the caller rolls the speech state back
        (`rollback_speech_state`) - phase B touches nothing else that survives (x2 is rewritten by the embed phase)."""
        with torch.cuda.stream(self.stream):
            self._set_forced(forced)
            self._phase_A(tok_start, tok_diff, q)
            self.token_host.copy_(self.token_dev, non_blocking=True)
            self._tok_event.record(self.stream)
            dn = self._noise_in(noise, sde_noise, frame)      # frame: device noise, as in step_speech
            self.spec_slot = self._speech(float(self.cfg_scale), stage, dn)     # ring slot of the speculative frame's chunk (stage), or None
        if on_enqueued is not None:
            on_enqueued()          # e.g. hand the previous frame's audio to the streamer: it completes before this step's token
        self._tok_event.synchronize()
        return int(self.token_host[0])

    def __del__(self):
        try:
            if self._own_stream:
                self.stream.synchronize()
                _IDLE_STREAMS.setdefault(str(self.device), []).append(self.stream)
        except Exception:      # noqa: BLE001  (interpreter shutdown)
            pass

    def decode_begin(self, tok_start: int, tok_diff: int, forced: Optional[int], spec_noise=None, q=None, spec_frame: Optional[int] = None):
        """Lock-step batches (one Engine per sample, one host loop): enqueue phase A - and, with `spec_noise` = (noise, sde_noise), the
        speculative phase B behind it - without waiting; `decode_end` returns the token.  `q`: the token is drawn on the device (step_decode).
        spec_frame: the speculative phase B with device noise, drawn for that frame index."""
        with torch.cuda.stream(self.stream):
            self._set_forced(forced)
            self._phase_A(tok_start, tok_diff, q)
            self.token_host.copy_(self.token_dev, non_blocking=True)
            self._tok_event.record(self.stream)
            if spec_frame is not None:
                self._upload_frame(spec_frame)
                self._run("B", self._seq_B, float(self.cfg_scale), "dn")
            elif spec_noise is not None:
                self._upload_noise(*spec_noise)
                self._run("B", self._seq_B, float(self.cfg_scale))

    def decode_end(self) -> int:
        self._tok_event.synchronize()
        return int(self.token_host[0])

    def stage_chunk(self) -> int:
        """Enqueue the async D2H copy of the frame just generated into the next ring slot; returns the slot."""
        k = self._ring_n % len(self._ring)
        self._ring_n += 1
        with torch.cuda.stream(self.stream):
            self._ring[k].copy_(self.wav, non_blocking=True)
            self._ring_ev[k].record(self.stream)
        return k

    def take_chunk(self, k: int) -> torch.Tensor:
        """Wait for slot k's copy and return its samples (a fresh CPU tensor: the slot is reused seven frames later)."""
        self._ring_ev[k].synchronize()
        return self._ring[k].clone()

    def rollback_speech_state(self):
        """Undo the streaming-state updates of the last phase B (a mis-speculated frame)."""
        blob = self.w.state_blob()
        with torch.cuda.stream(self.stream):
            self._ck(self.lib.vv_copy_rows(self._state_snap.data_ptr(), blob.numel(), blob.data_ptr(), blob.numel(), 1, blob.numel(), self.sp), "rollback")

    def step_embed(self):
        with torch.cuda.stream(self.stream):
            self._run("C", self._seq_C)

    # ---------------------------------------------------------------------------------------------------------
    # voice-prompt path (runs once per utterance)
    # ---------------------------------------------------------------------------------------------------------
    def acoustic_encode(self, wav: torch.Tensor, stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        """Whole-utterance (non-streaming) acoustic encoder: wav [T] -> mean latents [ceil(T/hop), vae_dim].  `stream`: run on another HIP
        stream (the encoder of a voice prompt is stateless: the voices of a dialogue encode concurrently, see acoustic_encode_many)."""
        T = wav.shape[0]
        F = (T + self.cfg.hop - 1) // self.cfg.hop
        st = stream or self.stream
        with torch.cuda.stream(st):
            x = wav.to(device=self.device, dtype=torch.float32).contiguous()
            ws = torch.empty(self.lib.vv_convnet_ws_bytes(C.byref(self.w.ac_enc), T, 0), dtype=torch.uint8, device=self.device)
            out = torch.empty(F, self.cfg.ac_dim, dtype=torch.float32, device=self.device)
            self._ck(self.lib.vv_encoder_forward(C.byref(self.w.ac_enc), x.data_ptr(), T, out.data_ptr(), ws.data_ptr(), st.cuda_stream),
                     "vv_encoder_forward")
        return out

    def acoustic_encode_many(self, wavs: List[torch.Tensor], max_streams: int = 4, side_streams: Optional[list] = None) -> List[torch.Tensor]:
        """The S voice prompts of a dialogue (modeling_vibevoice_inference.py:149-163 encodes them as one padded batch).  Each voice is an
        independent causal sequence with its own zero left context and its own ragged tail, so they are not stacked into the row
        dimension of one launch sequence (every conv / mixer would need per-segment halos); instead they run CONCURRENTLY on up to
        `max_streams` HIP streams over the shared weights: a single voice's late stages (T <= 200 rows) leave most CUs idle and its ~300
        launches are latency chains, which the other voices' chains fill.  Streams come from the recycle pool (engine.py, _IDLE_STREAMS)."""
        if len(wavs) <= 1:
            return [self.acoustic_encode(w) for w in wavs]
        pool = _IDLE_STREAMS.setdefault(str(self.device), [])
        n_side = min(max_streams, len(wavs)) - 1
        # side_streams: streams the caller already owns (the lanes of a batch) are used before any is taken from the pool or created: with the
        # lanes holding the pooled streams, every batched call would otherwise create three more (8 hardware queues: a batch of 5 on the lanes
        # dropped from 62 to 35 audio-sec/s after a batch of 2 had run first)
        lent, seen = [], {self.stream.cuda_stream}
        for st in (side_streams or []):
            if st.cuda_stream not in seen and len(lent) < n_side:
                lent.append(st)
                seen.add(st.cuda_stream)
        own = [pool.pop() if pool else torch.cuda.Stream(self.device) for _ in range(n_side - len(lent))]
        side = lent + own
        streams = [self.stream] + side
        outs = []
        try:
            for st in side:
                st.wait_stream(self.stream)                 # inputs were produced on / ordered into the engine stream
            for i, w in enumerate(wavs):
                st = streams[i % len(streams)]
                o = self.acoustic_encode(w, stream=st)
                if st is not self.stream:
                    o.record_stream(self.stream)
                outs.append(o)
        finally:                                            # streams go back to the pool whatever happened (they are never just dropped)
            for st in side:
                self.stream.wait_stream(st)
            pool.extend(own)
        return outs

    def connector(self, which: str, x: torch.Tensor) -> torch.Tensor:
        c = self.w.ac_conn if which == "acoustic" else self.w.sem_conn
        R = x.shape[0]
        with torch.cuda.stream(self.stream):
            x = x.to(device=self.device, dtype=torch.float32).contiguous()
            out = torch.empty(R, self.cfg.hidden, dtype=torch.float32, device=self.device)
            ws = torch.empty(R, self.cfg.hidden, dtype=torch.float32, device=self.device)
            self._ck(self.lib.vv_connector_forward(C.byref(c), x.data_ptr(), R, out.data_ptr(), 0, ws.data_ptr(), self.sp), "connector")
        return out

    def embed_ids(self, ids: torch.Tensor) -> torch.Tensor:
        with torch.cuda.stream(self.stream):
            return self.w.embed[ids.to(self.device)].float()

    def close(self):
        self._drop_graphs()
