"""First-chunk latency with and without a prepared voice prefix (voice_prefix.py), one workload per process.
python tools/mb_voice_prefix.py [cfg2|cfg3] [--runs N] [--step-limit SECONDS]      (profiles/voice_prefix.txt)

cfg2 is BASELINE.json's headline workload (1.5B, one 203-frame voice, 330 prompt tokens), cfg3 the 4-speaker one.  Timed as
bench.py::first_chunk_leg does: generate() entry -> first 3200-sample chunk on the host through an AudioStreamer, p50 / min / max; the two
variants alternate inside one loop, after one warm-up call of each.  The legs come from HIP events on the engine stream as in
bench.py::first_chunk_parts (median): voice encode, full prefill, suffix prefill (restore included), the vv_kv_copy restore alone, and the
one-off prepare_voice_prefix (events around the whole call, the final synchronise included).  Every timed step has a limit of its own
(SIGALRM, --step-limit): it ends the process with a non-zero status when a step is slow, but a Python signal handler only runs between
bytecodes, so it cannot interrupt a step that hangs inside a blocking HIP call.  Run the tool under an outer limit as well, one process per
workload:   timeout -k 10 300 python tools/mb_voice_prefix.py cfg2"""
import argparse
import ctypes as C
import os
import signal
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from vibevoice_rocm_amd import _lib as L  # noqa: E402
from vibevoice_rocm_amd.config import VVConfig  # noqa: E402
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference  # noqa: E402
from vibevoice_rocm_amd.streamer import AudioStreamer  # noqa: E402
from vibevoice_rocm_amd.synth import synth_state_dict_torch  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="cfg2", choices=["cfg2", "cfg3"])
ap.add_argument("--runs", type=int, default=15)
ap.add_argument("--step-limit", type=int, default=60)
args = ap.parse_args()


class StepLimit(Exception):
    pass


def _alarm(signum, frame):
    raise StepLimit()


signal.signal(signal.SIGALRM, _alarm)


def limited(what, fn):
    signal.alarm(args.step_limit)
    try:
        return fn()
    except StepLimit:
        print(f"{what}: exceeded its {args.step_limit} s limit", flush=True)
        os._exit(3)
    finally:
        signal.alarm(0)


w = bench.WORKLOADS[args.workload]
cfg = VVConfig.preset(w["model"])
sd = synth_state_dict_torch(cfg, 1234, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(w["steps"])
wl = bench.build_workload(cfg, 4, w["voice_frames"], speakers=w["speakers"], text=w["text"], turn=0)
eng = m.engine
ids, mask = wl["input_ids"][0], wl["speech_input_mask"][0]
L0 = int(ids.numel())
P = L0 - (w["text"] + 1)              # build_workload: everything before the script tokens and the final speech_start depends on the voices alone
assert not bool(mask[P:].any())
forced = [wl["special"]["speech_diffusion"]] * 2 + wl["forced"][-2:]
common = dict(input_ids=wl["input_ids"], tokenizer=wl["tok"], cfg_scale=1.3, forced_tokens=forced, noise=wl["noise"], speech_input_mask=wl["speech_input_mask"],
              generation_config={"do_sample": False})
full_kw = dict(speech_tensors=wl["speech_tensors"], speech_masks=wl["speech_masks"], speech_noise=wl["speech_noise"])


class Timer(AudioStreamer):
    def __init__(self):
        super().__init__(batch_size=1)
        self.t_first = None

    def put(self, audio_chunks, sample_indices):
        audio_chunks[0].detach().cpu()
        if self.t_first is None:
            self.t_first = time.perf_counter()


def first_chunk(**kw):
    st = Timer()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.generate(audio_streamer=st, **common, **kw)
    return 1e3 * (st.t_first - t0), out


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(eng.stream):
        e0.record(eng.stream)
        r = fn()
        e1.record(eng.stream)
    eng.stream.synchronize()
    return e0.elapsed_time(e1), r


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def prepare():
    return m.prepare_voice_prefix(ids[:P], wl["speech_tensors"], wl["speech_masks"], mask[:P], speech_noise=wl["speech_noise"])


print(f"== {args.workload}: {w['model']} bf16, {w['speakers']} speaker(s) x {w['voice_frames']} voice frames, prompt {L0} tokens = prefix {P} + script {L0 - P}; "
      f"{torch.cuda.get_device_name(0)}; {args.runs} runs per figure, the two variants alternating", flush=True)

# warm-up: one call of each variant (kernels loaded, graphs captured, caches sized), and one prepare
_, ref = limited("warm-up, full prompt", lambda: first_chunk(**full_kw))
vp = limited("warm-up, prepare_voice_prefix", prepare)
_, got = limited("warm-up, prefix", lambda: first_chunk(voice_prefix=vp))
a, b = ref.speech_outputs[0][0].double().cpu(), got.speech_outputs[0][0].double().cpu()
same = ref.sequences.tolist() == got.sequences.tolist()
print(f"store: {vp.nbytes / 2 ** 20:.2f} MiB ({cfg.layers} layers x {cfg.kv_heads} KV heads x {vp.kv.s_max} slots x {cfg.head_dim}, k and v, {vp.dtype}); "
      f"outputs with / without prefix: sequences {'equal' if same else 'DIFFER'}, waveform rel RMS {float((a - b).pow(2).mean().sqrt() / a.pow(2).mean().sqrt()):.2e}", flush=True)

lat = {"full": [], "prefix": []}
for _ in range(args.runs):
    lat["full"].append(limited("first chunk, full prompt", lambda: first_chunk(**full_kw))[0])
    lat["prefix"].append(limited("first chunk, prefix", lambda: first_chunk(voice_prefix=vp))[0])
sf, sp = stats(lat["full"]), stats(lat["prefix"])
print("first chunk, generate() entry -> first 3200-sample chunk on the host [ms]      p50     min     max")
print(f"  full prompt (voice encode + {L0}-row prefill + first frame)            {sf[0]:8.2f}{sf[1]:8.2f}{sf[2]:8.2f}")
print(f"  voice prefix (restore + {L0 - P}-row prefill + first frame)               {sp[0]:8.2f}{sp[1]:8.2f}{sp[2]:8.2f}")
saving, spread = sf[0] - sp[0], max(sf[2] - sf[1], sp[2] - sp[1])
print(f"  saving at p50: {saving:.2f} ms ({100 * saving / sf[0]:.0f} %); largest min-max spread of the two rows: {spread:.2f} ms -> "
      f"{'the saving is larger than the spread' if saving > spread else 'THE SAVING IS NOT LARGER THAN THE SPREAD OF THE RUNS'}", flush=True)

# the legs, HIP events on the engine stream
vt = wl["speech_tensors"].to(eng.device).float()
V = cfg.vocab
x_full = torch.randn(L0, cfg.hidden, device=eng.device) * 0.02
x_suf = x_full[P:].contiguous()
neg = eng.embed_ids(torch.tensor([V - 4]))
eng.begin_sequence(L0 + 64, [V - 4, V - 3, V - 2, V - 1])
eng.stream.synchronize()
legs = {
    "voice encode (_process_speech_inputs)": lambda: m._process_speech_inputs(vt, wl["speech_masks"], *wl["speech_noise"]),
    f"full prefill, {L0} + 1 rows": lambda: eng.prefill(x_full, row=0, pos0=0, neg_embed=neg),
    f"suffix prefill, {L0 - P} + 1 rows at position {P}, restore included": lambda: eng.prefill(x_suf, row=0, pos0=0, neg_embed=neg, prefix=vp),
    f"vv_kv_copy restore of {P} slots alone": lambda: L.check(eng.lib.vv_kv_copy(C.byref(vp.kv), 0, C.byref(eng.kv), 0, P, eng.sp), "vv_kv_copy"),
}
res = {}
for name, fn in legs.items():
    limited(name + " (warm-up)", lambda: event_ms(fn))
    res[name] = stats([limited(name, lambda: event_ms(fn))[0] for _ in range(args.runs)])
one_off = stats([limited("prepare_voice_prefix", lambda: event_ms(prepare))[0] for _ in range(5)])
print("legs, HIP events on the engine stream [ms]                                       p50     min     max")
for name, s in res.items():
    print(f"  {name:<76}{s[0]:8.3f}{s[1]:8.3f}{s[2]:8.3f}")
print(f"  {'prepare_voice_prefix, one-off (encode + prefix prefill + copy + synchronise), 5 runs':<76}{one_off[0]:8.3f}{one_off[1]:8.3f}{one_off[2]:8.3f}")
names = list(res)
expect = res[names[0]][0] + res[names[1]][0] - res[names[2]][0]
print(f"expected from the legs: voice encode + (full - suffix prefill) = {expect:.2f} ms; measured end to end: {saving:.2f} ms; "
      f"the voice-encode leg alone: {res[names[0]][0]:.2f} ms -> the saving is {'at least' if saving >= res[names[0]][0] else 'LESS THAN'} that leg", flush=True)
eng.stream.synchronize()
