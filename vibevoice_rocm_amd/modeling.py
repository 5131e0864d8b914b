"""Host-side mirror of the reference's inference class on top of the MI355X engine.

`VibeVoiceForConditionalGenerationInference` keeps the call surface `demo/inference_from_file.py` (and the Gradio
apps) use — `from_pretrained(path, torch_dtype=, device_map=, attn_implementation=)`, `.eval()`,
`.set_ddpm_inference_steps(num_steps=)`, `.generate(**processor_outputs, max_new_tokens=None, cfg_scale=,
tokenizer=, generation_config={'do_sample': False}, verbose=, audio_streamer=, stop_check_fn=, ...)`,
`.model.language_model.config._attn_implementation`, `.ddpm_inference_steps`, `.device`, `.model.noise_scheduler` —
and returns the same `VibeVoiceGenerationOutput(sequences, speech_outputs, reach_max_step_sample)`
(reference: vibevoice/modular/modeling_vibevoice_inference.py:38-51,68-147,326-693).
`_generate_one` restates :364-693 for one utterance on one engine; a batch runs through the one batched loop of batchloop.py, which drives
the dialogues through `_LaneDriver` (one Engine lane each) or `_RowDriver` (row batches, rowbatch.py).
"""
from __future__ import annotations

import json
import os
from types import SimpleNamespace
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from . import batchloop
from . import voice_prefix as VP
from .batchloop import VibeVoiceGenerationOutput, _BatchCoupling      # noqa: F401  (public names of this module)
from .config import VVConfig
from .engine import Engine, check_kv_cache_dtype
from .synth import state_dict_shapes
from .weights import MXFP6_ROWS_MAX_HIDDEN
from .voice_prefix import VoicePrefix      # noqa: F401  (public name of this module)

LANES_IN_FLIGHT = 4       # lock-step batches: lanes (one HIP stream each) enqueued concurrently; see _LaneDriver


def _read_safetensors_dir(path: str) -> Dict[str, torch.Tensor]:
    from safetensors.torch import load_file
    idx = os.path.join(path, "model.safetensors.index.json")
    files = []
    if os.path.exists(idx):
        with open(idx) as f:
            files = sorted(set(json.load(f)["weight_map"].values()))
    elif os.path.exists(os.path.join(path, "model.safetensors")):
        files = ["model.safetensors"]
    else:
        raise FileNotFoundError(f"no model.safetensors[.index.json] under {path}")
    sd: Dict[str, torch.Tensor] = {}
    for fn in files:
        sd.update(load_file(os.path.join(path, fn)))
    return sd


def load_state_dict_from_dir(path: str) -> Dict[str, torch.Tensor]:
    """HF sharded-safetensors checkpoint as the reference's converter writes it
    (vibevoice/scripts/convert_nnscaler_checkpoint_to_transformers.py:116-123).  Plain tensors only: a pre-quantized bitsandbytes checkpoint is
    refused here (load_prequantized_dir reads it)."""
    sd = _read_safetensors_dir(path)
    bnb = [k for k in sd if k.endswith((".weight.absmax", ".weight.quant_map", ".weight.quant_state.bitsandbytes__nf4",
                                        ".weight.quant_state.bitsandbytes__fp4", ".weight.nested_absmax"))]
    if bnb:
        raise NotImplementedError(f"{path!r} is a pre-quantized bitsandbytes 4-bit checkpoint ({bnb[0]!r}, ...): this plain-tensor loader does not "
                                  "read it. Use load_prequantized_dir(path), which returns the plain tensors and the NF4 matrices as they are, or "
                                  "VibeVoiceForConditionalGenerationInference.from_pretrained(path), which detects the format and runs it as "
                                  "weight_quant='nf4'")
    return sd


def load_prequantized_dir(path: str):
    """(plain tensors, {weight key: bnb.BnbNF4}) of a checkpoint directory: a pre-quantized bitsandbytes NF4 checkpoint (what save_pretrained
    writes after a BitsAndBytesConfig(load_in_4bit=True, bnb_4bit_quant_type="nf4") load; format in bnb.py) gives its quantised matrices as
    records and every other tensor as it is; a plain checkpoint gives an empty record dict."""
    from .bnb import split_prequantized
    return split_prequantized(_read_safetensors_dir(path))


def weight_quant_from_config(quantization_config, weight_quant: Optional[str] = None) -> Optional[str]:
    """Map a transformers BitsAndBytesConfig - or any object or dict with its attribute names - onto this engine's weight_quant.
    load_in_4bit with bnb_4bit_quant_type "nf4" -> "nf4" (weights and activations stay bf16 whatever torch_dtype / bnb_4bit_compute_dtype says:
    the engine has no fp16 path; bnb_4bit_use_double_quant is accepted, the block scales stay fp32).  fp4 and 8-bit loads are not built."""
    if quantization_config is None:
        return weight_quant

    def get(name, default=None):
        if isinstance(quantization_config, dict):
            return quantization_config.get(name, default)
        return getattr(quantization_config, name, default)

    built = "built: 4-bit NF4 (load_in_4bit=True, bnb_4bit_quant_type='nf4', or weight_quant='nf4'), weight-only fp8 (weight_quant='fp8'), weight-only OCP MXFP4 (weight_quant='mxfp4') and weight-only OCP MXFP6 e2m3 (weight_quant='mxfp6')"
    if get("load_in_8bit", False):
        raise NotImplementedError(f"load_in_8bit is not built; {built}")
    if not get("load_in_4bit", False):
        raise NotImplementedError(f"quantization_config without load_in_4bit is not built; {built}")
    qt = str(get("bnb_4bit_quant_type", "fp4")).lower()     # bitsandbytes' default 4-bit type is fp4
    if qt != "nf4":
        raise NotImplementedError(f"bnb_4bit_quant_type={qt!r} is not built; {built}")
    if weight_quant not in (None, "nf4"):
        raise ValueError(f"quantization_config asks for nf4 but weight_quant={weight_quant!r}: give one or the other")
    return "nf4"


def save_checkpoint_dir(path: str, config: VVConfig, state_dict: Dict[str, torch.Tensor], max_shard_bytes: int = 2 * 10 ** 9,
                        language_model_pretrained_name: str = "Qwen/Qwen2.5-1.5B") -> None:
    """Write a checkpoint directory in the layout the reference's converter produces
    (vibevoice/scripts/convert_nnscaler_checkpoint_to_transformers.py:92-123): `config.json` in the reference's schema (incl. the
    `vibepod_*` model_type keys of vibevoice/configs/*.json), `preprocessor_config.json`, and safetensors shards of at most
    `max_shard_bytes` with `model.safetensors.index.json` (a single `model.safetensors` when everything fits one shard).
    Tied checkpoints carry no `lm_head.weight` (HF save_pretrained drops the alias)."""
    from safetensors.torch import save_file
    os.makedirs(path, exist_ok=True)
    j = config.to_reference_json()
    j["model_type"] = "vibepod"
    j["acoustic_tokenizer_config"]["model_type"] = "vibepod_acoustic_tokenizer"
    j["semantic_tokenizer_config"]["model_type"] = "vibepod_semantic_tokenizer"
    j["diffusion_head_config"]["model_type"] = "vibepod_diffusion_head"
    j["torch_dtype"] = j["decoder_config"]["torch_dtype"] = "bfloat16"
    j["tie_word_embeddings"] = bool(config.tie)             # the converter passes it to VibeVoiceConfig (:46-50)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(j, f, indent=2, sort_keys=True)
    with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
        json.dump({"processor_class": "VibeVoiceProcessor", "speech_tok_compress_ratio": config.hop, "db_normalize": True,
                   "audio_processor": {"feature_extractor_type": "VibeVoiceTokenizerProcessor", "sampling_rate": 24000,
                                       "normalize_audio": True, "target_dB_FS": -25, "eps": 1e-6},
                   "language_model_pretrained_name": language_model_pretrained_name}, f, indent=2)
    names = [k for k in state_dict if not (config.tie and k == "lm_head.weight")]
    shards, cur, cur_bytes = [], {}, 0
    for k in names:
        t = state_dict[k].detach().cpu().contiguous()
        nb = t.numel() * t.element_size()
        if cur and cur_bytes + nb > max_shard_bytes:
            shards.append(cur)
            cur, cur_bytes = {}, 0
        cur[k] = t
        cur_bytes += nb
    shards.append(cur)
    if len(shards) == 1:
        save_file(shards[0], os.path.join(path, "model.safetensors"), metadata={"format": "pt"})
        return
    weight_map, total = {}, 0
    for i, sh in enumerate(shards):
        fn = f"model-{i + 1:05d}-of-{len(shards):05d}.safetensors"
        save_file(sh, os.path.join(path, fn), metadata={"format": "pt"})
        for k, t in sh.items():
            weight_map[k] = fn
            total += t.numel() * t.element_size()
    with open(os.path.join(path, "model.safetensors.index.json"), "w") as f:
        json.dump({"metadata": {"total_size": total}, "weight_map": weight_map}, f, indent=2)


def _copy_kv_slot(k: torch.Tensor, v: torch.Tensor, vt: Optional[torch.Tensor], row: int, src: int, dst: int) -> None:
    """slot src -> slot dst of KV cache row `row` in every layer ([layers, rows, kv_heads, s_max, head_dim]; vt: the transposed value
    copy in 32-key tiles [layers, rows, kv_heads, s_max / 32, head_dim, 32])"""
    k[:, row, :, dst].copy_(k[:, row, :, src])
    v[:, row, :, dst].copy_(v[:, row, :, src])
    if vt is not None:
        vt[:, row, :, dst // 32, :, dst % 32].copy_(vt[:, row, :, src // 32, :, src % 32])


def _warped_probs(gen_cfg: dict):
    """logits -> fp32 probabilities of the do_sample path (modeling_vibevoice_inference.py:491-494): the HF warpers the reference's callers
    configure (temperature, top_k, top_p; main.py:1187-1196) in HF order, softmax in fp64.  The device-side sampler (vv_sampler in
    include/vv_hip.h) restates exactly this arithmetic."""
    temperature, top_k, top_p = batchloop.sampler_params(gen_cfg)

    def probs(logits: torch.Tensor) -> torch.Tensor:
        z = logits.double() / temperature
        if 0 < top_k < z.numel():
            kth = torch.topk(z, top_k).values[-1]
            z = torch.where(z < kth, torch.full_like(z, float("-inf")), z)
        if top_p < 1.0:
            sz, order = torch.sort(z, descending=False)
            cum = torch.softmax(sz, -1).cumsum(-1)
            remove = cum <= (1 - top_p)
            remove[-1] = False
            z[order[remove]] = float("-inf")
        return torch.softmax(z, -1).float()
    return probs


def _make_sampler(gen_cfg: dict):
    """do_sample path on the host: the warped probabilities of the 4-5 valid logits (_warped_probs) + multinomial from torch's CPU generator."""
    probs = _warped_probs(gen_cfg)

    def sample(logits: torch.Tensor, ids):
        return ids[int(torch.multinomial(probs(logits), 1))]
    return sample


def _cfg_scales(cfg_scale, B: int) -> Optional[List[float]]:
    """generate(cfg_scale=): None for a scalar (today's path), the B floats of a sequence (one guidance scale per dialogue); ValueError when
    their number is not the batch's."""
    if isinstance(cfg_scale, (list, tuple)) or (isinstance(cfg_scale, (torch.Tensor, np.ndarray)) and cfg_scale.ndim > 0):
        rows = [float(c) for c in cfg_scale]
        if len(rows) != B:
            raise ValueError(f"cfg_scale: {len(rows)} guidance scales for {B} dialogues (a number, or one per dialogue)")
        return rows
    return None


def _embed_prompt(eng: Engine, ids: torch.Tensor, voice, after: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
    """Prompt embeddings of one dialogue on eng's stream, the voice rows `(mask, rows)` scattered over their placeholders (`after`: the
    stream that produced the rows)."""
    with torch.cuda.stream(eng.stream):
        x0 = eng.embed_ids(ids)
        if voice is not None:
            if after is not None:
                eng.stream.wait_stream(after)
            x0[voice[0].to(eng.device)] = voice[1]                                              # :221-224
    return x0


PACKED_PREFILL_ROWS = 4096      # rows per packed prefill pass (packed_prefill_rows=): eight headline prompts, their negative rows included, are one pass


def check_packed_rows(rows) -> int:
    if isinstance(rows, bool) or not isinstance(rows, int) or rows < 64:
        raise ValueError(f"packed_prefill_rows={rows!r}: an int >= 64 (rows per packed prefill pass)")
    return rows


class _LaneDriver:
    """batchloop driver: one Engine lane per dialogue (own HIP stream, KV cache and conv state).  Phase A of every live sample is enqueued
    before any token is awaited, so the B dependent chains fill each other's bubbles on the GPU; a sample is the same computation as in a
    batch of one - bit for bit with injected noise."""

    def __init__(self, model, B: int, cfg_scale, ST: int, SD: int):
        """cfg_scale: a number, or B of them - every lane then runs with its own scalar"""
        rows = _cfg_scales(cfg_scale, B)
        self.model, self.cfg_scale, self.ST, self.SD = model, (rows or [float(cfg_scale)] * B), ST, SD
        self.lanes = [model._lane(b) for b in range(B)]
        self.prefixes = [None] * B          # generate(voice_prefix=): dialogue -> VoicePrefix or None
        self.packed = None                  # packed_prefill: rows per pass - every lane's prompt then runs through vv_llm_prefill_packed (Engine.prefill)
        for e in self.lanes[1:]:
            e.sync_in()
        self.sde, self.n_steps = self.lanes[0].sde, self.lanes[0].n_steps
        self.dn = False                     # set_noise_seeds: `eligible` / `speech` rows are (frame index, None), the lanes draw the noise
        self.pool = None
        if os.environ.get("VV_LANE_THREADS", "1") != "0":
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=min(B, LANES_IN_FLIGHT))

    def begin(self, prompts, voices, max_steps, valid):
        self.x0 = []
        for eng, ids, voice, vp, scale in zip(self.lanes, prompts, voices, self.prefixes, self.cfg_scale):
            eng.cfg_scale = scale
            eng.begin_sequence(len(ids) + max(max_steps, 1) + 8, valid)
            if vp is not None:
                ids, voice = ids[vp.P:], None           # the rows after the prefix; every voice row lies inside it (VP.check)
            self.x0.append(_embed_prompt(eng, ids, voice, after=self.model.engine.stream))     # conn_all was produced on lane 0's stream

    def set_sampler(self, temperature, top_k, top_p):
        for e in self.lanes:
            e.set_sampler(temperature, top_k, top_p)

    def set_noise_seeds(self, seeds):
        self.dn = True
        for e, sd in zip(self.lanes, seeds):
            e.set_noise_seed(sd)

    def set_token_sampling(self, samplers, seeds):
        for e, row, sd in zip(self.lanes, samplers, seeds):
            e.set_sampler_row(0, *row)
            e.set_token_seeds([sd])

    def first_tokens(self, live, forced, sample_fn, q=None):
        lanes, toks = self.lanes, {}
        for b in live:
            lanes[b].prefill(self.x0[b], row=0, pos0=0, chunk=self.packed or getattr(self.model, "_prefill_chunk", 1024),
                             neg_embed=lanes[b].embed_ids(torch.tensor([self.ST])), prefix=self.prefixes[b], packed=self.packed is not None)
        for b in live:
            toks[b] = lanes[b].first_token(self.ST, self.SD, forced[b], sample_fn, q=(q or {}).get(b))
            if toks[b] == self.SD:
                lanes[b].commit_negative_prompt()
        return toks

    def decode(self, live, forced, eligible, sample_fn, deliver, q=None):
        lanes, q = self.lanes, q or {}
        if sample_fn is not None:
            deliver()                  # step_decode waits inside: the previous step's chunks go out ahead of it
            return {b: lanes[b].step_decode(self.ST, self.SD, forced[b], sample_fn) for b in live}, set()
        # a frame is ~600 graph nodes and the runtime enqueues them node by node: the lanes' launches go out from one host
        # thread each (the HIP calls release the GIL), or the host becomes the bottleneck at batch > 2
        # at most LANES_IN_FLIGHT lanes run at once: more streams than that serialise badly on MI355X (8 streams in flight are
        # slower than 4), so lane b of a larger batch shares the HIP stream of lane b % LANES_IN_FLIGHT and stream order queues
        # it behind that lane's frame.  One host thread per stream (never two threads on one stream: first use captures graphs).
        def begin(s_):
            for b in live:
                if b % LANES_IN_FLIGHT == s_:
                    if self.dn:
                        lanes[b].decode_begin(self.ST, self.SD, forced[b], q=q.get(b), spec_frame=eligible[b][0] if b in eligible else None)
                    else:
                        lanes[b].decode_begin(self.ST, self.SD, forced[b], eligible.get(b), q=q.get(b))
        slots = sorted({b % LANES_IN_FLIGHT for b in live})
        if self.pool is not None and len(slots) > 1:
            list(self.pool.map(begin, slots))
        else:
            for s_ in slots:
                begin(s_)
        deliver()                      # the previous step's chunks: their copies completed long before this step's tokens
        return {b: lanes[b].decode_end() for b in live}, set(eligible)

    def replace_negative(self, b, src, dst):
        e = self.lanes[b]
        with torch.cuda.stream(e.stream):
            _copy_kv_slot(e._kv_t[0], e._kv_t[1], e._kv_vt if e.kv.vt else None, 1, src, dst)

    def rollback(self, b):
        self.lanes[b].rollback_speech_state()

    def reset_speech(self, b):
        with torch.cuda.stream(self.lanes[b].stream):
            self.lanes[b].reset_speech_caches()

    def embed(self, b):
        self.lanes[b].step_embed()

    def finished(self, b):
        pass

    def speech(self, rows):
        for b, (n_row, s_row) in rows.items():
            if self.dn:
                self.lanes[b].step_speech(None, None, frame=n_row)
            else:
                self.lanes[b].step_speech(n_row, s_row)

    def chunk(self, b):
        with torch.cuda.stream(self.lanes[b].stream):
            return self.lanes[b].wav.clone()

    def stage_chunk(self, b):
        return self.lanes[b].stage_chunk()

    def take_chunk(self, b, slot):
        return self.lanes[b].take_chunk(slot)

    def synchronize(self):
        for e in self.lanes:
            e.stream.synchronize()

    def close(self):
        if self.pool is not None:
            self.pool.shutdown()


ROW_BATCH_WIDTHS = (4, 8)      # dialogues per row batch at most: 8 rows (csrc gemv_rows_kernel) or 16 (gemv_rows16_kernel, bf16 weights only)


def check_row_batch_width(width, torch_dtype, weight_quant, kv_cache_dtype):
    """ValueError unless width is 4, or 8 on what the 16-row matrix-core GEMV serves: bf16 weights without companions, a bf16 KV cache"""
    if isinstance(width, bool) or width not in ROW_BATCH_WIDTHS:
        raise ValueError(f"row_batch_width={width!r}: 4 (row batches of up to 4 dialogues, 8 rows) or 8 (up to 8 dialogues, 16 rows)")
    if width == 8:
        if weight_quant is not None:
            raise ValueError(f"row_batch_width=8 serves bf16 weights only: the 16-row matrix-core GEMV has no weight_quant={weight_quant!r} form")
        if torch_dtype != torch.bfloat16:
            raise ValueError(f"row_batch_width=8 needs torch_dtype=torch.bfloat16, not {torch_dtype}")
        if kv_cache_dtype == "fp8":
            raise ValueError("row_batch_width=8 needs a bf16 KV cache: the row-batched decode step has no kv_cache_dtype='fp8' form")
    return int(width)


def check_batched_conv_rows(flag, torch_dtype, weight_quant, config):
    """ValueError unless the row-batched conv tails (batched_conv_rows=True, csrc/vv_conv_hot.hip) serve the model: bf16 weights without
    companions and tokenizers whose one-row stage is C = 2048 (32 filters, six ratios)"""
    if not flag:
        return False
    if weight_quant is not None:
        raise ValueError(f"batched_conv_rows=True serves bf16 weights only: the row-batched one-row stage has no weight_quant={weight_quant!r} form")
    if torch_dtype != torch.bfloat16:
        raise ValueError(f"batched_conv_rows=True needs torch_dtype=torch.bfloat16, not {torch_dtype}")
    for what, filt, ratios in (("acoustic decoder", config.ac_dec_filters, config.ac_ratios), ("semantic encoder", config.sem_filters, config.sem_ratios)):
        if filt != 32 or filt * 2 ** len(ratios) != 2048:
            raise ValueError(f"batched_conv_rows=True needs tokenizers whose one-row stage is C = 2048 (n_filters = 32): the {what} has n_filters = {filt}")
    return True


def row_partition(B: int, width: int = 4) -> List[int]:
    """Sizes of the row batches B dialogues run as: ceil(B / width) groups, balanced, the larger ones first (6 at width 4: [3, 3]; at 8: [6])"""
    n_groups = -(-B // width)
    return [B // n_groups + (1 if g < B % n_groups else 0) for g in range(n_groups)]


class _RowDriver:
    """batchloop driver: the B dialogues batched into the ROW dimension of the weight-heavy half of a frame (rowbatch.RowBatch: one Qwen2
    decode step with 2 B rows, one diffusion sampling with 2 B rows; the conv tokenizers stay per dialogue on their lanes' streams).  5..16
    dialogues run as ceil(B / 4) row batches (row_batch_width=8: 5..8 as one, 9..16 as two), all on the main stream: each step enqueues A and H of every batch, then the conv tails - a
    batch's tails overlap the other batches' A and H.  With do_sample every row batch's logits are read back once per step and the tokens
    drawn in ascending dialogue order, so a seeded call draws what the lanes draw; results agree with the lanes to the rounding of the
    matrix-core GEMV (activations as bf16 hi + lo, ~2e-6 relative per product)."""

    def __init__(self, model, B: int, cfg_scale, ST: int, SD: int, width: Optional[int] = None):
        """cfg_scale: a number (the scale is a launch argument of graph H and part of its key), or B of them: every row batch keeps its
        dialogues' scales on the device and runs the graph H that reads them there (RowBatch.begin(cfg_rows=)).  width: dialogues per row
        batch at most (default: the model's row_batch_width)"""
        self.width = int(getattr(model, "row_batch_width", 4) if width is None else width)
        self.cfg_rows = _cfg_scales(cfg_scale, B)
        self.model, self.main, self.cfg_scale, self.ST, self.SD = model, model.engine, (1.0 if self.cfg_rows else float(cfg_scale)), ST, SD
        if B > 4:
            # two row batches: no dialogue's conv tail on the main stream (lanes 0, 4, 8, ... live there) - the main stream then runs A and H of
            # the two batches back to back while all tails run beside it on the three side streams (8 dialogues: 108 -> 119 audio-sec/s, 6: 88 -> 99)
            self.lanes = [model._lane(i) for i in [i for i in range(3 * B) if i % LANES_IN_FLIGHT][:B]]
        else:
            self.lanes = [model._lane(b) for b in range(B)]
        self.sde, self.n_steps = self.lanes[0].sde, self.lanes[0].n_steps
        self.groups, self.at = [], {}          # (row batch, its dialogues); dialogue -> (row batch, index in it)
        self.dn = False                        # set_noise_seeds: `eligible` / `speech` rows are (frame index, None), graph H draws the noise
        self.prefixes = [None] * B             # generate(voice_prefix=): dialogue -> VoicePrefix or None
        self.packed = None                     # packed_prefill: rows per pass - first_tokens prefills a row batch's dialogues in one weight pass
        # batched_conv_rows: every row batch runs the one-row stage of both tokenizers once for its dialogues (RowBatch.enable_conv_rows)
        self.conv_rows = bool(getattr(model, "batched_conv_rows", False))

    def begin(self, prompts, voices, max_steps, valid):
        from .rowbatch import RowBatch
        model, lanes, B, off = self.model, self.lanes, len(self.lanes), 0
        for n in row_partition(B, self.width):                                                      # row batches of <= width dialogues, sizes balanced
            idxs = list(range(off, off + n))
            key = (n, off) if lanes[0] is model._lanes[0] else (n, off, "side")
            if self.conv_rows:
                key += ("conv_rows",)
            rb = model._rowbatch.get(key)
            if rb is None:
                rb = model._rowbatch[key] = RowBatch([lanes[b] for b in idxs], stream=self.main.stream)
                if self.conv_rows:
                    rb.enable_conv_rows()
            rb.begin(max(len(prompts[b]) for b in idxs) + max(max_steps, 1) + 8, valid, self.cfg_scale,
                     cfg_rows=[self.cfg_rows[b] for b in idxs] if self.cfg_rows else None)
            self.groups.append((rb, idxs))
            for b in idxs:
                self.at[b] = (rb, b - off)
            off += n
        self.x0 = [_embed_prompt(self.main, ids, voice) if vp is None else _embed_prompt(self.main, ids[vp.P:], None)
                   for ids, voice, vp in zip(prompts, voices, self.prefixes)]

    def set_sampler(self, temperature, top_k, top_p):
        for rb, _ in self.groups:
            rb.set_sampler(temperature, top_k, top_p)

    def set_noise_seeds(self, seeds):
        self.dn = True
        for rb, idxs in self.groups:
            rb.set_noise_seeds([seeds[b] for b in idxs])

    def set_token_sampling(self, samplers, seeds):
        for rb, idxs in self.groups:
            for loc, b in enumerate(idxs):
                rb.set_sampler_row(loc, *samplers[b])
            rb.set_token_seeds([seeds[b] for b in idxs])

    def first_tokens(self, live, forced, sample_fn, q=None):
        at, toks = self.at, {}
        st_embed = self.main.embed_ids(torch.tensor([self.ST]))
        if self.packed is not None:
            for rb, idxs in self.groups:       # one packed prefill per row batch: its live dialogues' prompts (and negative rows) share the weight passes
                mine = [b for b in idxs if b in live]
                if mine:
                    rb.prefill_packed([(at[b][1], self.x0[b], self.prefixes[b]) for b in mine], chunk_rows=self.packed, neg_embed=st_embed)
        else:
            for b in live:
                at[b][0].prefill(at[b][1], self.x0[b], chunk=getattr(self.model, "_prefill_chunk", 1024), neg_embed=st_embed, prefix=self.prefixes[b])
        for b in live:
            rb, loc = at[b]
            toks[b] = rb.first_token(loc, forced[b], sample_fn, q=(q or {}).get(b))
            if toks[b] == self.SD:
                rb.commit_negative(loc)
        return toks

    def decode(self, live, forced, eligible, sample_fn, deliver, q=None):
        at, ST, SD, q = self.at, self.ST, self.SD, q or {}
        loc = {b: at[b][1] for b in live}
        plan = [(rb, [b for b in idxs if b in forced]) for rb, idxs in self.groups]
        plan = [(rb, lv) for rb, lv in plan if lv]
        toks, speculated = {}, set()
        if sample_fn is not None:
            # do_sample: A1 of every row batch, ONE wait for all their logits, the tokens drawn in ascending dialogue order (the lanes' order),
            # then A2 with them as forced tokens.  No speculation (the token is known only once the host has drawn it), as on the lanes
            for rb, lv in plan:
                rb.decode_logits()
            deliver()
            lg = {}
            for rb, lv in plan:
                lh = rb.logits_end()
                lg.update({b: lh[loc[b]] for b in lv})
            for b in live:
                rb = at[b][0]
                toks[b] = forced[b] if forced[b] is not None else int(sample_fn(lg[b][: len(rb.valid_ids)].clone(), rb.valid_ids))
            for rb, lv in plan:
                rb.decode_commit(ST, SD, {loc[b]: toks[b] for b in lv})
            return toks, speculated
        # graph A of every row batch; a batch in its steady state (every live dialogue diffusing, noise injected) gets its diffusion
        # sampling enqueued speculatively behind it.  The conv tails follow once all A / H are queued: each batch's tails are enqueued
        # when ITS sampler has finished (RowBatch.speech_tails) and run while the main stream works on the next batch
        for rb, lv in plan:
            rb.decode_begin(ST, SD, {loc[b]: forced[b] for b in lv}, q={loc[b]: q[b] for b in lv if b in q})
            if all(b in eligible for b in lv):
                if self.dn:
                    rb.speech_begin([loc[b] for b in lv], None, None, frames={loc[b]: eligible[b][0] for b in lv})
                else:
                    rb.speech_begin([loc[b] for b in lv], {loc[b]: eligible[b][0] for b in lv}, {loc[b]: eligible[b][1] for b in lv} if self.sde else None)
                speculated.update(lv)
        deliver()                      # the previous step's chunks (their copies completed long ago), before the host waits for a sampler
        for rb, lv in plan:
            if lv[0] in speculated:
                rb.speech_tails([loc[b] for b in lv])
        for rb, lv in plan:
            tk = rb.decode_end()
            toks.update({b: tk[loc[b]] for b in lv})
        return toks, speculated

    def replace_negative(self, b, src, dst):
        rb, loc = self.at[b]
        with torch.cuda.stream(rb.stream):
            _copy_kv_slot(rb._kv_t[0], rb._kv_t[1], rb._kv_vt if rb.kv.vt else None, 2 * loc + 1, src, dst)

    def rollback(self, b):
        self.at[b][0].rollback(self.at[b][1])

    def reset_speech(self, b):
        self.at[b][0].reset_speech(self.at[b][1])

    def embed(self, b):
        self.at[b][0].embed(self.at[b][1])

    def finished(self, b):
        self.at[b][0].set_active(self.at[b][1], False)

    def speech(self, rows):
        for rb, idxs in self.groups:
            mine = [b for b in idxs if b in rows]
            if mine:
                loc = {b: self.at[b][1] for b in mine}
                if self.dn:
                    rb.speech([loc[b] for b in mine], None, None, frames={loc[b]: rows[b][0] for b in mine})
                else:
                    rb.speech([loc[b] for b in mine], {loc[b]: rows[b][0] for b in mine}, {loc[b]: rows[b][1] for b in mine} if self.sde else None)
        for rb, _ in self.groups:
            rb.flush()                 # the conv tails are enqueued from worker threads: the chunk copies must queue behind them

    def chunk(self, b):
        with torch.cuda.stream(self.lanes[b].stream):
            return self.lanes[b].wav.clone()

    def stage_chunk(self, b):
        return self.lanes[b].stage_chunk()

    def take_chunk(self, b, slot):
        return self.lanes[b].take_chunk(slot)

    def synchronize(self):
        for rb, _ in self.groups:
            rb.synchronize()

    def close(self):
        pass


class _SessionDriver(_RowDriver):
    """batchloop.Session's driver: the row batches of _RowDriver with `slots` dialogues' worth of rows, opened once (`open`: KV caches sized
    for max_context tokens per dialogue, cache keys of their own in model._rowbatch) and refilled slot by slot (`admit`).  Every row batch keeps its
    slots' guidance scales on the device, so one graph H serves whatever scales its occupants bring."""

    def __init__(self, model, slots: int, ST: int, SD: int, device_noise: bool, packed: Optional[int] = None):
        super().__init__(model, slots, [1.0] * slots, ST, SD)
        self.packed = packed
        self.dn = bool(device_noise)
        self.x0 = [None] * slots

    def open(self, max_context: int, valid):
        from .rowbatch import RowBatch
        model, lanes, B, off = self.model, self.lanes, len(self.lanes), 0
        for n in row_partition(B, self.width):                                                      # as _RowDriver.begin partitions a batch
            idxs = list(range(off, off + n))
            key = (n, off, "session") if lanes[0] is model._lanes[0] else (n, off, "session", "side")
            if self.conv_rows:
                key += ("conv_rows",)
            rb = model._rowbatch.get(key)
            if rb is None:
                rb = model._rowbatch[key] = RowBatch([lanes[b] for b in idxs], stream=self.main.stream)
                if self.conv_rows:
                    rb.enable_conv_rows()
            rb.begin(max_context, valid, 1.0, cfg_rows=[1.0] * n)
            for loc in range(n):
                rb.set_active(loc, False)              # a free slot's rows are computed and dropped; its positions stay
            self.groups.append((rb, idxs))
            for b in idxs:
                self.at[b] = (rb, b - off)
            off += n

    def admit(self, b, req):
        rb, loc = self.at[b]
        rb.admit(loc, req.cfg_scale, req.noise_seed if self.dn else None, sampler=req.sampler, token_seed=req.token_seed)
        vp = self.prefixes[b] = req.prefix
        self.x0[b] = _embed_prompt(self.main, req.prompt, req.voice) if vp is None else _embed_prompt(self.main, req.prompt[vp.P:], None)

    def decode(self, live, forced, eligible, sample_fn, deliver, q=None):
        for rb, idxs in self.groups:
            for b in idxs:
                rb.set_active(self.at[b][1], b in forced)      # who is not in this step (free, or retired without an EOS) does not advance
        return super().decode(live, forced, eligible, sample_fn, deliver, q=q)

    def synchronize(self, b=None):
        if b is None:
            return super().synchronize()
        self.at[b][0].flush()
        self.lanes[b].stream.synchronize()


class VibeVoiceSession:
    """An open serving session of one model (model.open_session): dialogues are submitted one by one, each with its own guidance scale, limits,
    schedule, noise seed and streamer; `step()` admits queued dialogues into free row-batch slots and advances every live one by a token.  Each
    dialogue is served as generate() serves it alone (batchloop.Session).  The sampler (generation_config, device_sampling) and the solver are
    the session's - opened with seeded_tokens=True, every request may bring its own generation_config and token_seed instead (submit) -; admission is synchronous (a newcomer's prefill runs between two steps on the main stream;
    opened with packed_prefill=True, the requests queued at a step are admitted together and their prompts prefilled in one weight pass per row batch)."""

    def __init__(self, model, tokenizer, slots, max_context, generation_config, device_noise, device_sampling, seeded_tokens=False,
                 packed_prefill=False):
        self.model, cfg = model, model.config
        gen_cfg = dict(generation_config or {})
        do_sample = bool(gen_cfg.get("do_sample", False))
        on_device = model.device_sampling if device_sampling is None else bool(device_sampling)
        self.seeded_tokens = bool(seeded_tokens)
        if self.seeded_tokens:
            if device_sampling is not None and not device_sampling:
                raise ValueError("open_session(): seeded_tokens=True draws the tokens on the device: device_sampling=False cannot go with it")
            on_device = True
            if do_sample:
                batchloop.sampler_row(gen_cfg)             # ValueError for warpers the kernels do not take
        sampler = batchloop.sampler_params(gen_cfg) if do_sample and on_device else None
        sample_fn = _make_sampler(gen_cfg) if do_sample and sampler is None else None
        self.special = dict(speech_start=tokenizer.speech_start_id, speech_end=tokenizer.speech_end_id, speech_diffusion=tokenizer.speech_diffusion_id,
                            eos=tokenizer.eos_token_id, bos=getattr(tokenizer, "bos_token_id", None))
        pad_id = getattr(tokenizer, "pad_id", None)
        self.driver = _SessionDriver(model, slots, self.special["speech_start"], self.special["speech_diffusion"], device_noise,
                                     packed=model.packed_prefill_rows if packed_prefill else None)
        model.engine.sync_in()
        with torch.cuda.stream(model.engine.stream):
            self.driver.open(int(max_context), batchloop.valid_token_ids(self.special))
            self._s = batchloop.Session(self.driver, slots, self.special, self.special["eos"] if pad_id is None else pad_id, cfg.max_pos, cfg.latent,
                                        max_context, device_noise=device_noise, sample_fn=sample_fn, sampler=sampler,
                                        speculate=model.speculative_frames and model._use_graphs, on_close=self._closed,
                                        seeded_tokens=self.seeded_tokens, packed_prefill=bool(packed_prefill))

    slots = property(lambda self: self._s.slots)
    admission_ms = property(lambda self: self._s.admission_ms)      # host time of every admission (prefill + first token, synchronous): the stall of the running dialogues
    closed = property(lambda self: self._s.closed)

    @torch.no_grad()
    def submit(self, input_ids=None, attention_mask=None, speech_tensors=None, speech_masks=None, speech_input_mask=None, cfg_scale: float = 1.0,
               max_new_tokens: Optional[int] = None, max_length_times=2, forced_tokens=None, noise=None, sde_noise=None, noise_seed=None,
               voice_prefix=None, audio_streamer=None, stop_check_fn=None, speech_noise=None, generation_config=None,
               token_seed=None) -> batchloop.SessionHandle:
        """Queue one dialogue (the arguments generate() takes for a batch of one) and return its handle.  The voice encode - or the restore of its
        voice_prefix - runs here; nothing else does.  ValueError when prompt + step limit + 8 exceeds the session's max_context (nothing is
        clipped), and for noise= / sde_noise= in a device-noise session.  In a session opened with seeded_tokens=True, generation_config= gives this
        request its own do_sample / temperature / top_k / top_p (None: the session's) and token_seed= its own token seed (None: drawn here, after the
        noise seed); in any other session either raises ValueError."""
        model = self.model
        input_ids = torch.as_tensor(input_ids)
        in_dev = input_ids.device
        input_ids = input_ids.cpu()
        if input_ids.dim() == 1:
            input_ids = input_ids[None]
        if input_ids.shape[0] != 1:
            raise ValueError(f"submit(): one dialogue per request, not a batch of {input_ids.shape[0]}")
        attention_mask = torch.ones_like(input_ids) if attention_mask is None else torch.as_tensor(attention_mask).cpu().reshape(1, -1)
        keep = attention_mask[0].bool()
        ids = input_ids[0][keep]
        req = batchloop.SessionRequest(prompt=ids, head=input_ids[0][~keep], cfg_scale=float(cfg_scale), max_new_tokens=max_new_tokens,
                                       max_length_times=max_length_times, forced_tokens=forced_tokens,
                                       noise=None if noise is None else torch.as_tensor(noise), sde_noise=None if sde_noise is None else torch.as_tensor(sde_noise),
                                       noise_seed=noise_seed, audio_streamer=audio_streamer, stop_check_fn=stop_check_fn, in_dev=in_dev,
                                       sampler=None if generation_config is None or not self.seeded_tokens else batchloop.sampler_row(generation_config),
                                       token_seed=None if token_seed is None else int(token_seed) % 2 ** 64)
        if generation_config is not None and not self.seeded_tokens:
            raise ValueError("submit(generation_config=) needs a session opened with seeded_tokens=True (this session has one sampler)")
        self._s.validate(req)              # before any work on the device
        if speech_input_mask is not None:
            speech_input_mask = torch.as_tensor(speech_input_mask).cpu().reshape(1, -1)
        vps = VP.per_dialogue(voice_prefix, 1)
        for rb, _ in self.driver.groups:
            rb.flush()                     # the voice encode runs on the lanes' streams too: no worker thread may still be feeding one
        model.engine.sync_in()
        with torch.cuda.stream(model.engine.stream):
            if vps is not None:
                speech_tensors, speech_masks, speech_noise, speech_input_mask = model._apply_voice_prefixes(
                    vps, input_ids, attention_mask, speech_input_mask, speech_tensors, speech_masks, speech_noise)
                req.prefix = vps[0]
            if speech_tensors is not None and speech_masks is not None and speech_input_mask is not None:
                sp = speech_input_mask[0][keep].bool()
                if int(sp.sum()):
                    _, conn = model._process_speech_inputs(torch.as_tensor(speech_tensors).float(), torch.as_tensor(speech_masks).bool(), *(speech_noise or (None, None)))
                    req.voice = (sp, conn[: int(sp.sum())])
        return self._s.submit(req)

    @torch.no_grad()
    def step(self) -> bool:
        """One step of the session; False once nothing is live or queued."""
        eng = self.model.engine
        eng.sync_in()
        with torch.cuda.stream(eng.stream):
            return self._s.step()

    def run(self):
        while self.step():
            pass

    def close(self):
        with torch.cuda.stream(self.model.engine.stream):
            self._s.close()

    def _closed(self):
        self.model.engine.stream.synchronize()
        self.model._session = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class VibeVoiceForConditionalGenerationInference:
    def __init__(self, config: VVConfig, state_dict: Dict[str, torch.Tensor], device="cuda:0", torch_dtype=torch.bfloat16,
                 attn_implementation: str = "hip_gfx950", use_graphs: bool = True, weight_quant: Optional[str] = None, prequant=None,
                 kv_cache_dtype: Optional[str] = None, device_sampling: bool = False, device_noise: bool = False, mxfp4_row_batch: bool = False,
                 seeded_tokens: bool = False, row_batch_width: int = 4, packed_prefill: bool = False, packed_prefill_rows: int = PACKED_PREFILL_ROWS,
                 batched_conv_rows: bool = False, mxfp4_lean: bool = False, mxfp6_row_batch: bool = False, mxfp6_lean: bool = False):
        # batched_conv_rows: a row batch runs the one-row stage (C = 2048) of the acoustic decoder and the semantic encoder, and the connectors,
        # once for all its dialogues - one pass over 78 % of the tokenizers' weights instead of one per dialogue (csrc/vv_conv_hot.hip, DESIGN.md
        # section 5o).  bf16 weights without companions only.  Off by default; generate(batched_conv_rows=) overrides it per call, a session
        # inherits it; one dialogue and the lanes ignore it.  Checked first: a bad combination raises ValueError before any weight is touched
        self.batched_conv_rows = check_batched_conv_rows(batched_conv_rows, torch.bfloat16 if prequant else torch_dtype,
                                                         "nf4" if prequant else weight_quant, config)
        # packed_prefill: the prompts of a row batch's dialogues are prefilled in ONE weight pass (RowBatch.prefill_packed, vv_llm_prefill_packed)
        # instead of one pass per dialogue, in passes of at most packed_prefill_rows rows; a single dialogue and the lanes take the same entry
        # for their one prompt.  Off by default; generate(packed_prefill=, packed_prefill_rows=) overrides per call, open_session(packed_prefill=)
        # per session
        self.packed_prefill = bool(packed_prefill)
        self.packed_prefill_rows = check_packed_rows(packed_prefill_rows)
        # row_batch_width: dialogues per row batch at most.  4 (default): 5..16 dialogues run as ceil(B / 4) row batches of up to 8 rows.  8: as
        # ceil(B / 8) row batches of up to 16 rows - one pass over the LLM and head weights for up to 8 dialogues (csrc gemv_rows16_kernel; bf16
        # weights and KV cache only; DESIGN.md section 5m says for which batch sizes that is faster).  generate(row_batch_width=) overrides it per call
        self.row_batch_width = check_row_batch_width(row_batch_width, torch.bfloat16 if prequant else torch_dtype, "nf4" if prequant else weight_quant,
                                                     kv_cache_dtype)
        # kv_cache_dtype: None / "bf16" = the KV cache in the compute dtype; "fp8" = e4m3 bytes with one power-of-two scale per (layer, KV head)
        # for the decode steps (bf16 arithmetic, head_dim 128; the prompt is prefilled on a bf16 staging cache and converted, engine.py); combines
        # with any weight_quant.  Checked first: a bad value raises ValueError before any weight is touched
        check_kv_cache_dtype(kv_cache_dtype, torch.bfloat16 if prequant else torch_dtype, config.head_dim)
        self.kv_cache_dtype = kv_cache_dtype
        # prequant: the NF4 matrices of a pre-quantized bitsandbytes checkpoint ({weight key: bnb.BnbNF4}, load_prequantized_dir); they run as
        # weight_quant="nf4" with bf16 compute, codes and scales taken as the file holds them
        shapes = state_dict_shapes(config)
        if prequant:
            from .bnb import check_shapes
            check_shapes(prequant, shapes)
            if weight_quant not in (None, "nf4"):
                raise ValueError(f"a pre-quantized bitsandbytes NF4 checkpoint runs as weight_quant='nf4', not {weight_quant!r}")
            weight_quant, torch_dtype = "nf4", torch.bfloat16
        # mxfp4_row_batch=True (weight_quant="mxfp4" only): batches of row_batch_min..16 dialogues and serving sessions run the row-batched path on
        # fragment-major copies of the MXFP4 codes and scale bytes (csrc/vv_gemv_rows.hip; +0.53 B per copied weight).
        # Off by default: the batch then runs on the lanes and open_session refuses the mode, as before
        if mxfp4_row_batch and weight_quant != "mxfp4":
            raise ValueError(f"mxfp4_row_batch=True needs weight_quant='mxfp4', not {weight_quant!r}")
        self.mxfp4_row_batch = bool(mxfp4_row_batch)
        # mxfp4_lean=True (weight_quant="mxfp4" only): the LLM's matrices are held as MXFP4 codes alone - no bf16 copies - and the prompt passes
        # run a matrix-core GEMM on the codes (csrc/vv_gemm_mx.hip).  Memory is the point: -2 B per LLM weight.  Composes
        # with every other option of an mxfp4 model; without mxfp4_row_batch batches run on the lanes and sessions are refused, as without it
        if mxfp4_lean and weight_quant != "mxfp4":
            raise ValueError(f"mxfp4_lean=True needs weight_quant='mxfp4', not {weight_quant!r}")
        self.mxfp4_lean = bool(mxfp4_lean)
        # mxfp6_row_batch=True (weight_quant="mxfp6" only): batches of row_batch_min..4 dialogues per row batch and serving sessions run the
        # row-batched path on fragment-major copies of the MXFP6 codes and scale bytes (csrc/vv_gemv_rows_mx6.hip; +0.78 B
        # per copied weight).  Off by default: the batch then runs on the lanes and open_session refuses the mode, as before.  row_batch_width=8
        # and batched_conv_rows=True have refused every weight_quant above, this one included
        if mxfp6_row_batch and weight_quant != "mxfp6":
            raise ValueError(f"mxfp6_row_batch=True needs weight_quant='mxfp6', not {weight_quant!r}")
        if mxfp6_row_batch and config.hidden > MXFP6_ROWS_MAX_HIDDEN:
            raise ValueError(f"mxfp6_row_batch=True serves LLM hidden sizes up to {MXFP6_ROWS_MAX_HIDDEN}, not {config.hidden}")
        self.mxfp6_row_batch = bool(mxfp6_row_batch)
        # mxfp6_lean=True (weight_quant="mxfp6" only): the LLM's matrices are held as MXFP6 codes alone - no bf16 copies - and the prompt passes
        # run a matrix-core GEMM on the codes (csrc/vv_gemm_mx6.hip).  Memory is the point: -2 B per LLM weight.  Composes
        # with every other option of an mxfp6 model; without mxfp6_row_batch batches run on the lanes and sessions are refused, as without it
        if mxfp6_lean and weight_quant != "mxfp6":
            raise ValueError(f"mxfp6_lean=True needs weight_quant='mxfp6', not {weight_quant!r}")
        self.mxfp6_lean = bool(mxfp6_lean)
        missing = [k for k in shapes if k not in state_dict and k not in (prequant or {})]
        if missing:
            raise KeyError(f"state dict is missing {len(missing)} tensors, e.g. {missing[:4]}")
        self.config = config
        self.dtype = torch_dtype
        # launch a frame's diffusion tail right behind the LLM step while the host still waits for the token (rolled back when the
        # token is not speech_diffusion); results are identical either way (tests/test_hip_parity.py)
        self.speculative_frames = True
        # batches of 2..8 dialogues: one weight pass per frame for all of them (rowbatch.py) instead of one per dialogue (lanes)
        self.row_batch = os.environ.get("VV_ROW_BATCH", "1") != "0"
        self.row_batch_min = int(os.environ.get("VV_ROW_BATCH_MIN", "2"))      # 2 dialogues: 64 vs 58 audio-sec/s on the lanes
        self._rowbatch = {}
        self._session = None              # the open serving session (open_session), at most one
        # do_sample: draw the token inside the LLM step's tail launch from exponential draws the host makes before it enqueues the step
        # (vv_sampler), instead of reading the logits back for a host softmax / multinomial: one graph and one 4-byte read-back per token, and
        # speculative frame launch as for greedy decoding.  Seeded calls keep their tokens and the generator its state.  Off by default;
        # generate(..., device_sampling=...) overrides it per call
        self.device_sampling = bool(device_sampling)
        # diffusion noise drawn on the device (vv_noise_normal at the head of the frame's graph) as a function of (the dialogue's noise_seed,
        # frame, solver step, element) instead of torch.randn on the host in the reference's order: nothing but a frame index is uploaded, every
        # batched call may speculate its frames, and a dialogue sounds the same alone and in a batch.  Same distribution, another sequence than
        # the reference's RNG stream.  Off by default; generate(..., device_noise=..., noise_seed=...) overrides it per call
        self.device_noise = bool(device_noise)
        # do_sample tokens drawn on the device from a counter-based generator (vv_token_draws) as a function of (the dialogue's token_seed, the
        # position, its own logits), under warpers that are the dialogue's own row of a device array: one captured graph A serves dialogues with
        # different generation_configs - greedy ones too - and a dialogue's tokens are the same alone, on a lane, in a row batch or in a
        # session.  Implies device sampling.  Same distribution, another sequence than the reference's RNG stream.  Off by default;
        # generate(..., seeded_tokens=..., token_seed=...) overrides it per call
        self.seeded_tokens = bool(seeded_tokens)
        # weight_quant="fp8": weight-only e4m3 companions for the per-frame weight-streaming GEMVs;
        # "nf4": weight-only 4-bit NF4 companions for the same GEMVs (batches of >= 2 run on the lanes)
        # "mxfp4": weight-only OCP MXFP4 companions (e2m1 codes, one power-of-two scale byte per 32 k) decoded by the vector ALU's own
        # conversion instruction (batches of >= 2 run on the lanes, sessions refuse it - unless mxfp4_row_batch=True)
        # "mxfp6": weight-only OCP MXFP6 companions (e2m3 codes, 6.25 bits per weight: fp8's mantissa at 0.78 of its bytes), decoded 32 at a time
        # by v_cvt_scalef32_pk32_f32_fp6 (batches of >= 2 run on the lanes, sessions refuse it - unless mxfp6_row_batch=True)
        self.weight_quant = weight_quant
        self.engine = Engine(config, state_dict, device=device, dtype=torch_dtype, use_graphs=use_graphs, weight_quant=weight_quant,
                             prequant=prequant, kv_cache_dtype=kv_cache_dtype, mxfp4_row_batch=self.mxfp4_row_batch,
                             mxfp4_lean=self.mxfp4_lean, mxfp6_row_batch=self.mxfp6_row_batch, mxfp6_lean=self.mxfp6_lean)
        self.device = self.engine.device
        # batches run in lock step on one Engine per sample (own HIP stream, KV cache and conv state; matrices already in the streamed
        # dtype on the device are shared, not copied): lanes beyond the first are built on first use from this state dict
        self._lanes = [self.engine]
        self._use_graphs = use_graphs
        self.ddpm_inference_steps = config.ddpm_infer
        # attribute paths the reference's callers read
        lm_cfg = SimpleNamespace(_attn_implementation=attn_implementation, hidden_size=config.hidden,
                                 max_position_embeddings=config.max_pos)
        self.model = SimpleNamespace(language_model=SimpleNamespace(config=lm_cfg), noise_scheduler=self.engine.scheduler)

    # ---- construction ----------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=torch.bfloat16, device_map=None,
                        attn_implementation: Optional[str] = None, subfolder: Optional[str] = None, config=None, quantization_config=None,
                        local_files_only=None, cache_dir=None, **kw):
        """Load a local checkpoint directory (config.json + safetensors shards).  `attn_implementation` is accepted for
        call compatibility; attention always runs on the hand-written gfx950 kernel.  `subfolder` joins the path; `config` (the shim's
        VibeVoiceConfig, a VVConfig or a config.json dict) overrides the directory's config.json.  A pre-quantized bitsandbytes NF4 checkpoint
        is detected from its tensors, with or without `quantization_config`, and runs as weight_quant="nf4" in bf16.  `local_files_only` and
        `cache_dir` are accepted and ignored: paths are local directories only."""
        path = str(pretrained_model_name_or_path)
        if subfolder:
            path = os.path.join(path, subfolder)
        if not os.path.isdir(path):
            raise OSError(f"{path!r} is not a local checkpoint directory (this build has no hub access)")
        wq = weight_quant_from_config(quantization_config, kw.get("weight_quant"))
        if wq == "nf4" and quantization_config is not None:
            torch_dtype = torch.bfloat16        # bnb's fp16 / bf16 compute dtype is served as bf16 (no fp16 path)
        if config is None:
            cfg = VVConfig.from_pretrained(path)
        elif isinstance(config, VVConfig):
            cfg = config
        elif isinstance(config, dict):
            cfg = VVConfig.from_json_dict(config)
        else:
            cfg = VVConfig.from_json_dict(config.to_dict())
        sd, prequant = load_prequantized_dir(path)
        if prequant:
            if kw.get("weight_quant") not in (None, "nf4"):
                raise ValueError(f"{path!r} is a pre-quantized bitsandbytes NF4 checkpoint: weight_quant={kw.get('weight_quant')!r} cannot apply")
            wq, torch_dtype = "nf4", torch.bfloat16
        device = device_map if isinstance(device_map, (str, torch.device)) and str(device_map) not in ("auto", "cpu") else "cuda:0"
        if str(device) == "cuda":
            device = "cuda:0"
        return cls(cfg, sd, device=device, torch_dtype=torch_dtype, attn_implementation=attn_implementation or "hip_gfx950",
                   use_graphs=kw.get("use_graphs", True), weight_quant=wq, prequant=prequant or None, kv_cache_dtype=kw.get("kv_cache_dtype"),
                   device_sampling=kw.get("device_sampling", False), device_noise=kw.get("device_noise", False),
                   mxfp4_row_batch=kw.get("mxfp4_row_batch", False), seeded_tokens=kw.get("seeded_tokens", False),
                   row_batch_width=kw.get("row_batch_width", 4), packed_prefill=kw.get("packed_prefill", False),
                   packed_prefill_rows=kw.get("packed_prefill_rows", PACKED_PREFILL_ROWS), batched_conv_rows=kw.get("batched_conv_rows", False),
                   mxfp4_lean=kw.get("mxfp4_lean", False), mxfp6_row_batch=kw.get("mxfp6_row_batch", False), mxfp6_lean=kw.get("mxfp6_lean", False))

    @classmethod
    def from_synthetic(cls, config: VVConfig, seed: int = 1234, device="cuda:0", torch_dtype=torch.bfloat16, numpy_weights=False, **kw):
        """Random-init weights of the architecture (no checkpoints exist offline)."""
        from .synth import synth_state_dict, synth_state_dict_torch
        if numpy_weights:
            sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(config, seed).items()}
        else:
            sd = synth_state_dict_torch(config, seed, device=device, dtype=torch_dtype)
        return cls(config, sd, device=device, torch_dtype=torch_dtype, **kw)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def set_ddpm_inference_steps(self, num_steps=None):
        self.ddpm_inference_steps = num_steps or self.config.ddpm_infer
        # main.py:543-548 swaps the scheduler first: model.model.noise_scheduler = ....from_config(cfg, algorithm_type="sde-dpmsolver++", ...)
        if self.model.noise_scheduler is not self.engine.scheduler:
            self.engine.scheduler = self.model.noise_scheduler
        self.engine.set_steps(self.ddpm_inference_steps)

    @property
    def noise_scheduler(self):
        return self.engine.scheduler

    # ---- voice-prompt prefill --------------------------------------------------------------------------------
    def _process_speech_inputs(self, speech_tensors: torch.Tensor, speech_masks: torch.Tensor,
                               std_noise: Optional[torch.Tensor] = None, eps_noise: Optional[torch.Tensor] = None):
        """modeling_vibevoice_inference.py:149-163.  Returns (acoustic_features [S,F,64], connected [sum(mask), H])."""
        eng, cfg = self.engine, self.config
        with torch.cuda.stream(eng.stream):      # every torch op of the prefill rides the engine stream
            return self._process_speech_inputs_impl(speech_tensors, speech_masks, std_noise, eps_noise)

    def _process_speech_inputs_impl(self, speech_tensors, speech_masks, std_noise, eps_noise):
        eng, cfg = self.engine, self.config
        S, Tmax = speech_tensors.shape
        Fm = speech_masks.shape[1]
        n_frames = speech_masks.sum(-1).tolist()
        means = torch.zeros(S, Fm, cfg.ac_dim, dtype=torch.float32, device=self.device)
        # causal encoder: frames < n_frames[i] only see samples < n_frames[i]*hop, so the zero tail of the padded batch
        # row beyond that boundary never matters; when the boundary exceeds Tmax the reference pads features instead.
        t_len = [min(int(n_frames[i]) * cfg.hop, Tmax) for i in range(S)]
        live = [i for i in range(S) if t_len[i] > 0]
        with torch.cuda.stream(eng.stream):
            st_dev = speech_tensors.to(self.device)
        encoded = eng.acoustic_encode_many([st_dev[i, :t_len[i]] for i in live],      # the S voices run concurrently, on the lanes' streams if there are lanes
                                           side_streams=[e.stream for e in self._lanes[1:]])
        with torch.cuda.stream(eng.stream):
            for i, m in zip(live, encoded):
                means[i, : m.shape[0]] = m
        with torch.cuda.stream(eng.stream):
            if cfg.ac_std_dist == "gaussian":
                if std_noise is None:
                    std_noise = torch.randn(S, device=self.device, dtype=self.dtype)
                    eps_noise = torch.randn_like(torch.empty(S, cfg.ac_dim, Fm, device=self.device, dtype=self.dtype).permute(0, 2, 1))
                std = std_noise.to(self.device).float() * (cfg.ac_fix_std / 0.8)
                lat = means + std[:, None, None] * eps_noise.to(self.device).float()
            else:
                lat = means
            feats = (lat + eng.w.speech_bias) * eng.w.speech_scale
            sel = feats[speech_masks.to(self.device)]
        conn = eng.connector("acoustic", sel)
        return feats, conn

    # ---- voice prefix cache (voice_prefix.py) --------------------------------------------------------------------
    @torch.no_grad()
    def prepare_voice_prefix(self, input_ids, speech_tensors=None, speech_masks=None, speech_input_mask=None, speech_noise=None,
                             prefill_chunk: int = 1024) -> VoicePrefix:
        """The voice-only head of a prompt (`VibeVoiceProcessor.voice_prefix`), done once: the voice encode, the prefill of its P positions on the
        main engine - chunked as generate() chunks a prompt - and one vv_kv_copy of cache row 0 into a freshly allocated store.  The latents'
        noise (modeling_vibevoice_inference.py:149-163) is drawn here, once, or injected as `speech_noise` = (std_noise [S], eps_noise [S, F, 64]).
        Synchronises before it returns; the caller owns the VoicePrefix and hands it to generate(voice_prefix=...)."""
        eng = self.engine
        ids = torch.as_tensor(input_ids).cpu().long()
        if ids.dim() == 2 and ids.shape[0] == 1:
            ids = ids[0]
        if ids.dim() != 1 or ids.numel() == 0:
            raise ValueError(f"prepare_voice_prefix: input_ids must be one prefix ([P] or [1, P]), not shape {tuple(ids.shape)}")
        sp = None if speech_input_mask is None else torch.as_tensor(speech_input_mask).cpu().bool().reshape(-1)
        if sp is not None and sp.numel() != ids.numel():
            raise ValueError(f"prepare_voice_prefix: speech_input_mask has {sp.numel()} positions, input_ids {ids.numel()}")
        eng.sync_in()
        with torch.cuda.stream(eng.stream):
            voice = None
            if speech_tensors is not None and speech_masks is not None and sp is not None and int(sp.sum()):
                _, conn = self._process_speech_inputs(torch.as_tensor(speech_tensors).float(), torch.as_tensor(speech_masks).bool(), *(speech_noise or (None, None)))
                if conn.shape[0] != int(sp.sum()):
                    raise ValueError(f"prepare_voice_prefix: speech_input_mask marks {int(sp.sum())} positions, the voices have {conn.shape[0]} frames")
                voice = (sp, conn)
            x0 = _embed_prompt(eng, ids, voice)
            if eng.kv_fp8:
                kv, stage = eng.prefill(x0, chunk=int(prefill_chunk), keep_staging=True)      # the prompt's bf16 K / V, not their codes
                vp = eng.save_prefix(ids, kv=kv)
                del stage
            else:
                eng._ensure_kv(ids.numel())
                eng.prefill(x0, chunk=int(prefill_chunk))
                vp = eng.save_prefix(ids)
        return vp

    def _rows_quant_ok(self) -> bool:
        """the row-batched decode path serves this model's weights: bf16, weight-only fp8, or MXFP4 / MXFP6 with the fragment-major opt-in"""
        from .rowbatch import row_batch_ok
        return row_batch_ok(self.weight_quant, getattr(self, "mxfp4_row_batch", False), getattr(self, "mxfp6_row_batch", False))

    # ---- serving sessions ---------------------------------------------------------------------------------------
    def open_session(self, tokenizer=None, slots: int = 8, max_context: Optional[int] = None, generation_config=None, device_noise: bool = True,
                     device_sampling: Optional[bool] = None, seeded_tokens: bool = False, packed_prefill: bool = False) -> "VibeVoiceSession":
        """Open a serving session: `slots` (2..16) row-batch slots - ceil(slots / 4) row batches, as a batched generate() partitions them - whose
        KV caches are sized once for `max_context` tokens per dialogue (required).  Dialogues are submitted to the session one by one and a
        finished one frees its slot for the next between two steps (VibeVoiceSession, batchloop.Session).  Needs what row batching needs -
        bf16, weight_quant None or "fp8" (or "mxfp4" / "mxfp6" on a model built with mxfp4_row_batch=True / mxfp6_row_batch=True), a bf16 KV cache, graphs on - and raises ValueError otherwise: there is no lanes fallback.  One session
        per model; generate() raises RuntimeError until it is closed.  seeded_tokens=True: every request may bring its own generation_config and token_seed
        (submit), greedy and sampled requests share the one graph A, and a dialogue's tokens do not depend on who shares the session.
        packed_prefill=True: the requests queued when a step begins are admitted together and prefilled in one weight pass per row batch
        (passes of the model's packed_prefill_rows rows) instead of one pass each."""
        if getattr(self, "_session", None) is not None:
            raise RuntimeError("open_session(): this model already has an open session (one per model); close() it first")
        if tokenizer is None:
            raise ValueError("open_session() needs tokenizer= (for the speech_start/end/diffusion and eos ids)")
        if not isinstance(slots, int) or not 2 <= slots <= 16:
            raise ValueError(f"open_session(): slots={slots!r} (2..16)")
        if max_context is None or int(max_context) <= 0:
            raise ValueError("open_session(): max_context= (tokens per dialogue: prompt + generated + 8) is required")
        why = None
        if self.dtype != torch.bfloat16:
            why = f"torch_dtype={self.dtype} (bf16 only)"
        elif not self._rows_quant_ok():
            why = f"weight_quant={self.weight_quant!r} (None or 'fp8')"
        elif self.kv_cache_dtype == "fp8":
            why = "kv_cache_dtype='fp8' (the row-batched decode step has no fp8-KV form)"
        elif not self._use_graphs:
            why = "use_graphs=False (the session replays captured graphs)"
        if why is not None:
            raise ValueError(f"open_session(): a session runs on the row-batched decode path, which this model cannot take: {why}")
        sess = VibeVoiceSession(self, tokenizer, slots, int(max_context), generation_config, bool(device_noise), device_sampling, bool(seeded_tokens),
                                packed_prefill=bool(packed_prefill))
        self._session = sess
        return sess

    # ---- generation --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, input_ids: torch.Tensor = None, attention_mask: Optional[torch.Tensor] = None,
                 speech_tensors: Optional[torch.Tensor] = None, speech_masks: Optional[torch.Tensor] = None,
                 speech_input_mask: Optional[torch.Tensor] = None, tokenizer=None, generation_config=None,
                 max_new_tokens: Optional[int] = None, cfg_scale: float = 1.0, audio_streamer=None,
                 stop_check_fn: Optional[Callable[[], bool]] = None, return_speech: bool = True, **kwargs):
        if getattr(self, "_session", None) is not None:
            raise RuntimeError("generate(): a serving session is open on this model (its lanes and their conv state are the session's); close() it first")
        ids_ = torch.as_tensor(input_ids)
        rows_ = _cfg_scales(cfg_scale, 1 if ids_.dim() == 1 else int(ids_.shape[0]))      # ValueError before anything runs
        if rows_ is not None and len(rows_) == 1:
            cfg_scale = rows_[0]
        self._token_sampling_args(generation_config, kwargs, 1 if ids_.dim() == 1 else int(ids_.shape[0]))      # ValueError before anything runs
        self.engine.sync_in()
        with torch.cuda.stream(self.engine.stream):   # all torch glue (gathers, scatters, copies) rides the engine stream
            out = self._generate(input_ids, attention_mask, speech_tensors, speech_masks, speech_input_mask, tokenizer,
                                 generation_config, max_new_tokens, cfg_scale, audio_streamer, stop_check_fn, return_speech, **kwargs)
        self.engine.stream.synchronize()
        return out

    def _generate(self, input_ids, attention_mask, speech_tensors, speech_masks, speech_input_mask, tokenizer, generation_config,
                  max_new_tokens, cfg_scale, audio_streamer, stop_check_fn, return_speech, **kwargs):
        if tokenizer is None:
            raise ValueError("generate() needs tokenizer= (for the speech_start/end/diffusion and eos ids)")
        tok_rows = self._token_sampling_args(generation_config, kwargs, 1 if torch.as_tensor(input_ids).dim() == 1 else int(torch.as_tensor(input_ids).shape[0]))
        gen_cfg = dict((generation_config[0] if isinstance(generation_config, (list, tuple)) else generation_config) or {})
        do_sample = bool(gen_cfg.get("do_sample", False)) and tok_rows is None
        sampler = batchloop.sampler_params(gen_cfg) if do_sample and kwargs.get("device_sampling", self.device_sampling) else None
        sample_fn = _make_sampler(gen_cfg) if do_sample and sampler is None else None
        verbose = kwargs.get("verbose", False)
        max_length_times = kwargs.get("max_length_times", 2)
        refresh_negative = bool(kwargs.get("refresh_negative", True))     # False: reference :501-515 (no caller of the reference uses it)
        self._prefill_chunk = int(kwargs.get("prefill_chunk", 1024))   # extension: rows per prefill launch sequence (cfg 5: 512-token chunks)
        # extension: packed prompt prefill for this call (None: off), rows per pass
        packed = check_packed_rows(kwargs.get("packed_prefill_rows", self.packed_prefill_rows)) if kwargs.get("packed_prefill", self.packed_prefill) else None
        forced_tokens = kwargs.get("forced_tokens")          # extension: bench / fixtures drive the token schedule
        noise = kwargs.get("noise")                          # extension: injected diffusion noise [F, latent]
        speech_noise = kwargs.get("speech_noise")            # extension: (std_noise [S], eps_noise [S, F, 64])
        sde_noise = kwargs.get("sde_noise")                  # extension: injected variance noise of the SDE solver [F, n_steps, latent]
        noise = None if noise is None else torch.as_tensor(noise)
        sde_noise = None if sde_noise is None else torch.as_tensor(sde_noise)
        device_noise = bool(kwargs.get("device_noise", self.device_noise))      # extension: the diffusion noise is drawn on the device
        noise_seed = kwargs.get("noise_seed")                # with it: an int (dialogue b: seed + b), one int per dialogue, or None (drawn)
        if device_noise and (noise is not None or sde_noise is not None):
            raise ValueError("device_noise=True draws the diffusion noise on the device: noise= / sde_noise= cannot be injected with it")
        if noise_seed is not None and not device_noise:
            raise ValueError("noise_seed= seeds the device-side noise: it needs device_noise=True")
        input_ids = torch.as_tensor(input_ids)
        in_dev = input_ids.device                            # callers may hand over device tensors (the reference moves them itself, modeling_vibevoice_inference.py:288,305-307)
        input_ids = input_ids.cpu()                          # ids / masks drive host-side bookkeeping only
        if input_ids.dim() == 1:
            input_ids = input_ids[None]
        B, Lp = input_ids.shape
        noise_seeds = self._noise_seeds(noise_seed, B) if device_noise else None      # None: the call's first draw from the CPU generator
        # seeded token draws: the dialogues' sampler rows and token seeds (drawn, when not given, right after the noise seeds)
        token_sampling = None if tok_rows is None else (tok_rows, self._noise_seeds(kwargs.get("token_seed"), B, what="token_seed"))
        attention_mask = torch.ones_like(input_ids) if attention_mask is None else torch.as_tensor(attention_mask).cpu()
        if speech_input_mask is not None:
            speech_input_mask = torch.as_tensor(speech_input_mask).cpu()
        special = dict(speech_start=tokenizer.speech_start_id, speech_end=tokenizer.speech_end_id,
                       speech_diffusion=tokenizer.speech_diffusion_id, eos=tokenizer.eos_token_id,
                       bos=getattr(tokenizer, "bos_token_id", None))
        pad_id = getattr(tokenizer, "pad_id", None)
        if pad_id is None:
            pad_id = special["eos"]
        vps = VP.per_dialogue(kwargs.get("voice_prefix"), B)
        if vps is not None:
            speech_tensors, speech_masks, speech_noise, speech_input_mask = self._apply_voice_prefixes(
                vps, input_ids, attention_mask, speech_input_mask, speech_tensors, speech_masks, speech_noise)
        conn_all = None
        if speech_tensors is not None and speech_masks is not None:
            sn = speech_noise or (None, None)
            _, conn_all = self._process_speech_inputs(torch.as_tensor(speech_tensors).float(), torch.as_tensor(speech_masks).bool(), *sn)
        if B > 1:
            if not refresh_negative:
                # with refresh_negative=False the reference's batched loop couples the samples (a non-diffusing sample's negative step is
                # dropped only in steps where some OTHER sample diffuses, :588-622): served per sample here would not reproduce that
                raise NotImplementedError("refresh_negative=False is built for batch size 1 only")
            # dialogues batched into the row dimension of the LLM / diffusion-head weight passes (rowbatch.py), or one engine lane each
            rows = kwargs.get("row_batch", self.row_batch) and self.row_batch_min <= B <= 16 and self.dtype == torch.bfloat16 and \
                self._rows_quant_ok() and self.kv_cache_dtype != "fp8"      # fp8 KV: on the lanes (RowBatch needs a bf16 cache)
            if "row_batch_width" in kwargs:      # per call, like row_batch=: the same checks as at construction
                check_row_batch_width(kwargs["row_batch_width"], self.dtype, self.weight_quant, self.kv_cache_dtype)
            driver = (_RowDriver(self, B, cfg_scale, special["speech_start"], special["speech_diffusion"], width=kwargs.get("row_batch_width")) if rows
                      else _LaneDriver(self, B, cfg_scale, special["speech_start"], special["speech_diffusion"]))
            if vps is not None:
                driver.prefixes = vps
            driver.packed = packed
            if "batched_conv_rows" in kwargs:      # per call, like row_batch_width=: the same checks as at construction
                driver.conv_rows = check_batched_conv_rows(kwargs["batched_conv_rows"], self.dtype, self.weight_quant, self.config)
            call = batchloop.BatchCall(special=special, pad_id=pad_id, max_pos=self.config.max_pos, latent=self.config.latent,
                                       max_new_tokens=max_new_tokens, max_length_times=max_length_times, forced_tokens=forced_tokens, noise=noise,
                                       sde_noise=sde_noise, audio_streamer=audio_streamer, stop_check_fn=stop_check_fn, verbose=verbose,
                                       sample_fn=sample_fn, sampler=sampler, speculate=self.speculative_frames and self._use_graphs, return_speech=return_speech,
                                       in_dev=in_dev, noise_seeds=noise_seeds, token_sampling=token_sampling)
            try:
                return batchloop.run(driver, input_ids, attention_mask, speech_input_mask, conn_all, call)
            finally:
                driver.close()         # the lanes' host threads, also when the loop raises
        keep = attention_mask[0].bool()
        ids = input_ids[0][keep]                             # left padding carries no information (position_ids = cumsum(mask)-1)
        sp, conn = None, None
        if speech_input_mask is not None:
            sp = speech_input_mask[0][keep].bool()
            if int(sp.sum()) and conn_all is not None:
                conn = conn_all[: int(sp.sum())]
        r = self._generate_one(ids, sp, conn, special, cfg_scale, max_new_tokens, max_length_times, forced_tokens, noise, audio_streamer,
                               stop_check_fn, 0, verbose, sample_fn, sde_noise, refresh_negative=refresh_negative, sampler=sampler,
                               prefix=None if vps is None else vps[0], noise_seed=None if noise_seeds is None else noise_seeds[0],
                               token_sampling=None if token_sampling is None else (token_sampling[0][0], token_sampling[1][0]), packed=packed)
        if audio_streamer is not None:
            audio_streamer.end()
        return batchloop.pack_output([torch.cat([input_ids[0][~keep], r["sequence"]])], [r["audio"]], [r["reach_max"]], pad_id, in_dev, return_speech)

    def _token_sampling_args(self, generation_config, kwargs, B: int) -> Optional[List[tuple]]:
        """generate()'s seeded-token arguments, checked without touching the device or the generator.  Returns None when the call draws no token
        that way - seeded_tokens off, or do_sample false for every dialogue (nothing changes and nothing is drawn then) - else the B dialogues'
        sampler rows (batchloop.sampler_row).  ValueError: a generation_config list without seeded_tokens or of the wrong length, token_seed
        without seeded_tokens, seeded_tokens with device_sampling=False given explicitly, warpers the kernels do not take."""
        seeded = bool(kwargs.get("seeded_tokens", self.seeded_tokens))
        per = isinstance(generation_config, (list, tuple))
        if per and not seeded:
            raise ValueError("generation_config: one dict per dialogue needs seeded_tokens=True (a call has one sampler otherwise)")
        if per and len(generation_config) != B:
            raise ValueError(f"generation_config: {len(generation_config)} entries for {B} dialogues (a dict, or one per dialogue)")
        if kwargs.get("token_seed") is not None and not seeded:
            raise ValueError("token_seed= seeds the device-side token draws: it needs seeded_tokens=True")
        if not seeded:
            return None
        if kwargs.get("device_sampling") is not None and not kwargs.get("device_sampling"):
            raise ValueError("seeded_tokens=True draws the tokens on the device: device_sampling=False cannot go with it")
        if isinstance(kwargs.get("token_seed"), (list, tuple)) and len(kwargs["token_seed"]) != B:
            raise ValueError(f"token_seed: {len(kwargs['token_seed'])} seeds for {B} dialogues (an int, or one int per dialogue)")
        rows = [batchloop.sampler_row(g) for g in (generation_config if per else [generation_config] * B)]
        return rows if any(r != batchloop.GREEDY_ROW for r in rows) else None

    @staticmethod
    def _noise_seeds(noise_seed, B: int, what: str = "noise_seed") -> List[int]:
        """generate(device_noise=True, noise_seed=): the B dialogues' 64-bit seeds.  An int: dialogue b uses (seed + b) mod 2^64; a list of B
        ints: one each; None: B draws from torch's default CPU generator, so torch.manual_seed makes the call reproducible."""
        if noise_seed is None:
            return [int(v) for v in torch.randint(0, 2 ** 62, (B,))]
        if isinstance(noise_seed, (list, tuple)) or (isinstance(noise_seed, (torch.Tensor, np.ndarray)) and noise_seed.ndim > 0):
            seeds = [int(v) % 2 ** 64 for v in noise_seed]
            if len(seeds) != B:
                raise ValueError(f"{what}: {len(seeds)} seeds for {B} dialogues (an int, or one int per dialogue)")
            return seeds
        return [(int(noise_seed) + b) % 2 ** 64 for b in range(B)]

    def _apply_voice_prefixes(self, vps, input_ids, attention_mask, speech_input_mask, speech_tensors, speech_masks, speech_noise):
        """generate(voice_prefix=): every dialogue with a prefix is checked against it (VP.check: ValueError naming what differs) and loses its
        voice inputs - its voice rows are already in the store's K / V: its speech_input_mask row is cleared and its voices are not encoded.
        `speech_tensors` / `speech_masks` may be omitted when every dialogue has a prefix; otherwise they hold the voices of ALL dialogues, as the
        processor returns them for the batch, and the rows of the prefixed dialogues are skipped.  A dialogue's number of voices is the number
        of placeholder runs in its mask row.  Returns (speech_tensors, speech_masks, speech_noise, speech_input_mask)."""
        cfg, B = self.config, input_ids.shape[0]
        keep = attention_mask.bool()
        n_voices = []
        for b in range(B):
            sp_b = None if speech_input_mask is None else speech_input_mask[b][keep[b]].bool()
            if vps[b] is not None:
                dv = vps[b].k.device                # an index-less "cuda" is the current device: compare resolved indices
                if dv.type != self.device.type or dv.index != (torch.cuda.current_device() if self.device.index is None else self.device.index):
                    raise ValueError(f"voice_prefix: the store lives on {vps[b].k.device}, this model on {self.device}")
                VP.check(vps[b], input_ids[b][keep[b]], sp_b, cfg.layers, cfg.kv_heads, cfg.head_dim, self.engine.kv_dtype, where=f" (dialogue {b})" if B > 1 else "")
            n_voices.append(0 if sp_b is None or not sp_b.numel() else int((sp_b[1:] & ~sp_b[:-1]).sum()) + int(sp_b[0]))     # runs of True
        if speech_input_mask is not None:
            speech_input_mask = speech_input_mask.clone()
            for b in range(B):
                if vps[b] is not None:
                    speech_input_mask[b] = False
        full = [b for b in range(B) if vps[b] is None and n_voices[b]]
        if not full or speech_tensors is None or speech_masks is None:
            return (None, None, None, speech_input_mask) if not full else (speech_tensors, speech_masks, speech_noise, speech_input_mask)
        S = int(torch.as_tensor(speech_tensors).shape[0])
        if S != sum(n_voices):
            raise ValueError(f"voice_prefix: speech_tensors holds {S} voices, the dialogues' speech_input_mask rows mark {sum(n_voices)}: with a "
                             "per-dialogue list, give the voices of all dialogues as the processor returns them")
        first = [sum(n_voices[:b]) for b in range(B)]
        rows = torch.tensor([first[b] + i for b in full for i in range(n_voices[b])], dtype=torch.long)
        if speech_noise is not None:
            speech_noise = tuple(torch.as_tensor(t)[rows] for t in speech_noise)
        return torch.as_tensor(speech_tensors)[rows], torch.as_tensor(speech_masks)[rows], speech_noise, speech_input_mask

    # ---- batches: lock step over samples (batchloop.run through _LaneDriver / _RowDriver) -----------------------------------
    def release_lanes(self) -> None:
        """Drop the engines of earlier batched calls (lanes, row batches): their HIP streams go back to the recycle pool (engine.py, _IDLE_STREAMS)."""
        for rb in self._rowbatch.values():
            rb.close()
        self._rowbatch = {}
        for e in self._lanes[1:]:
            e.stream.synchronize()
            e.close()
        self._lanes = self._lanes[:1]

    def _lane(self, b: int) -> Engine:
        while len(self._lanes) <= b:
            n = len(self._lanes)             # lanes past LANES_IN_FLIGHT share the stream of lane n % LANES_IN_FLIGHT: see _LaneDriver
            eng = Engine(self.config, None, device=self.device, dtype=self.dtype, use_graphs=self._use_graphs, weight_quant=self.weight_quant, kv_cache_dtype=self.kv_cache_dtype,
                         stream=self._lanes[n % LANES_IN_FLIGHT].stream if n >= LANES_IN_FLIGHT else None, weights_from=self.engine)
            self._lanes.append(eng)
        eng = self._lanes[b]
        # a new lane starts on its own (ODE) schedule: taking over the main engine's scheduler goes through set_steps, which rebuilds the
        # solver tables (sde-dpmsolver++ included) - assigning the object alone would leave the lane's tables on the old solver
        if eng.scheduler is not self.engine.scheduler or eng.n_steps != self.engine.n_steps:
            eng.scheduler = self.engine.scheduler
            eng.set_steps(self.engine.n_steps)
        return eng

    def _generate_one(self, ids: torch.Tensor, sp_mask, conn, special, cfg_scale, max_new_tokens, max_length_times, forced_tokens,
                      noise, audio_streamer, stop_check_fn, sample_idx, verbose, sample_fn=None, sde_noise=None, refresh_negative=True, sampler=None,
                      prefix: Optional[VoicePrefix] = None, noise_seed: Optional[int] = None, token_sampling: Optional[tuple] = None,
                      packed: Optional[int] = None):
        eng, cfg = self.engine, self.config
        dn = noise_seed is not None         # device noise: the engine draws frame f's noise from (noise_seed, f); draw / pending_nz / rewind are not used
        nv = len(set(batchloop.valid_token_ids(special)))
        if sampler is not None:
            eng.set_sampler(*sampler)
        # device-side do_sample with drawn noise: a speculated frame's noise is drawn BEFORE its token is known.  Kept for the next frame after
        # a mis-speculation (the greedy rule) it would sit in front of the token draws in between and reorder the generator's sequence, so the
        # generator is put back to where it stood before the noise draw and the rows are dropped
        rewind = not dn and sampler is not None and (noise is None or (eng.sde and sde_noise is None))

        def draw(frame):
            """The frame's random draws, in the reference's order: randn(2, latent) for the initial latent (:699), then - SDE solver
            only - one randn(2, latent) per solver step (dpm_solver.py:993-998); rows [1:] never reach the result."""
            nz = noise[frame] if noise is not None else torch.randn(2, cfg.latent)[0]
            sz = None
            if eng.sde:
                sz = sde_noise[frame] if sde_noise is not None else torch.randn(eng.n_steps, 2, cfg.latent)[:, 0]
            return nz, sz

        ST, SE, SD, EOS = special["speech_start"], special["speech_end"], special["speech_diffusion"], special["eos"]
        # device-side position bookkeeping (vv_advance_lens): a negative "speech_start" id selects refresh_negative=False - the negative
        # row consumes every step's embedding and is never reset (:501-515); the batch-2 step computes that row anyway
        ST_dev = ST if refresh_negative else -1
        L0 = int(ids.shape[0])
        max_length, max_steps = batchloop.limits(cfg.max_pos, L0, max_new_tokens, max_length_times)
        eng.cfg_scale = float(cfg_scale)
        eng.begin_sequence(L0 + max(max_steps, 1) + 8, batchloop.valid_token_ids(special))
        if dn:
            eng.set_noise_seed(noise_seed)
        if token_sampling is not None:      # seeded token draws: (sampler row, token seed) - the steps take no q, the engine runs graph "Ar"
            eng.set_sampler_row(0, *token_sampling[0])
            eng.set_token_seeds([token_sampling[1]])
        # prefix: its P positions come out of the store; only the rows after it are embedded and prefilled (every voice row lies inside it)
        x0 = _embed_prompt(eng, ids, None if conn is None else (sp_mask, conn)) if prefix is None else _embed_prompt(eng, ids[prefix.P:], None)
        seq = ids.tolist()
        chunks: List[torch.Tensor] = []
        reach_max = False
        frame = 0
        stream_idx = torch.tensor([sample_idx])
        # speculative frame launch needs the token chosen on the device: greedy, forced, or sampled there (`sampler`); the host sampler
        # (sample_fn) needs the logits on the host first
        speculate = self.speculative_frames and sample_fn is None and eng.use_graphs
        prev_tok, pending_nz = None, None
        staged: List[int] = []          # ring slots whose audio has not been handed to the streamer yet (at most 2)

        def deliver():
            """Hand finished frames to the streamer.  Called right after the next step's launches are enqueued: the frame's copy
            completes before that step's token does, so waiting for it here delays nothing on the GPU."""
            while staged:
                audio_streamer.put(eng.take_chunk(staged.pop(0))[None, None], stream_idx)

        hook = deliver if audio_streamer is not None else None
        for step in range(max_steps):
            if stop_check_fn is not None and stop_check_fn():                                  # :432-438
                if verbose:
                    print(f"Generation stopped externally at step {step + 1}")
                if audio_streamer is not None:
                    deliver()
                    audio_streamer.end()
                break
            if audio_streamer is not None and hasattr(audio_streamer, "finished_flags") and audio_streamer.finished_flags[sample_idx]:
                break                                                                           # :441-445 (this sample's stream was ended externally)
            if len(seq) >= max_length:                                                          # :452-457
                reach_max = True
                break
            forced = forced_tokens[step] if (forced_tokens is not None and step < len(forced_tokens)) else None
            speculated = False
            q = batchloop.draw_q(nv) if (sampler is not None and forced is None) else None     # where the host sampler's multinomial draws
            if step == 0:
                # the negative branch's prompt, a single speech_start (:377-381), is one more row of the prompt prefill (cache row 1, position 0)
                eng.prefill(x0, row=0, pos0=0, chunk=packed or getattr(self, "_prefill_chunk", 1024), neg_embed=eng.embed_ids(torch.tensor([ST])), prefix=prefix,
                            packed=packed is not None)
                tok = eng.first_token(ST_dev, SD, forced, sample_fn, q=q)
                if tok == SD or not refresh_negative:
                    eng.commit_negative_prompt()         # the branch is in use from step 0 on (otherwise the row is overwritten by the next speech_start)
            elif dn and speculate and prev_tok == SD:
                # device noise: the speculated frame draws from its index; after a mis-speculation the next real frame has the same index and so
                # the same noise - nothing to keep, nothing to rewind
                tok = eng.step_decode_speculative(ST_dev, SD, forced, None, None, on_enqueued=hook, stage=audio_streamer is not None, q=q, frame=frame)
                speculated = True
                if tok != SD:
                    eng.rollback_speech_state()
            elif speculate and prev_tok == SD and (pending_nz is not None or ((noise is None or frame < len(noise)) and
                                                                            (sde_noise is None or frame < len(sde_noise)))):
                # steady state of a dialogue: the frame's diffusion tail is enqueued right behind the LLM step, the host waits
                # for the token only.  The noise row is the draw the reference makes when the token IS speech_diffusion; a draw
                # made for a mis-speculated frame is kept for the next real one (same RNG sequence).
                if pending_nz is None:
                    rng = torch.get_rng_state() if rewind else None
                    pending_nz = draw(frame)
                tok = eng.step_decode_speculative(ST_dev, SD, forced, *pending_nz, on_enqueued=hook, stage=audio_streamer is not None, q=q)
                speculated = True
                if tok != SD:
                    eng.rollback_speech_state()
                    if rewind:
                        torch.set_rng_state(rng)
                        pending_nz = None
            else:
                tok = eng.step_decode(ST_dev, SD, forced, sample_fn, on_enqueued=hook, q=q)          # :478-496 (+ speculative :581-583)
            prev_tok = tok
            seq.append(tok)
            if tok == EOS:                                                                      # :517-526
                if verbose:
                    print(f"Samples [{sample_idx}] reached EOS token at step {step + 1}.", flush=True)
                if audio_streamer is not None:
                    deliver()
                    audio_streamer.end(stream_idx)
                break
            if tok == SE:                                                                       # :540-544
                with torch.cuda.stream(eng.stream):
                    eng.reset_speech_caches()
            if tok == SD:                                                                       # :571-670
                slot = eng.spec_slot if speculated else None
                if not speculated and dn:
                    slot = eng.step_speech(None, None, stage=audio_streamer is not None, frame=frame)
                elif not speculated:
                    if pending_nz is None:
                        pending_nz = draw(frame)
                    slot = eng.step_speech(*pending_nz, stage=audio_streamer is not None)
                pending_nz = None
                with torch.cuda.stream(eng.stream):
                    chunk = eng.wav.clone()
                chunks.append(chunk)
                if audio_streamer is not None:
                    staged.append(slot if slot is not None else eng.stage_chunk())     # the copy went out right behind the acoustic decoder
                    if len(staged) > 2:
                        deliver()
                frame += 1
            else:
                eng.step_embed()                                                                # :567
        if audio_streamer is not None:
            deliver()
        eng.stream.synchronize()
        audio = torch.cat(chunks)[None] if chunks else None
        return dict(sequence=torch.tensor(seq, dtype=torch.long), audio=audio, reach_max=reach_max)
