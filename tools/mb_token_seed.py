"""Seeded token draws against today's device sampling, 1.5B shapes, bf16, in one process, the legs alternating after a warm-up of each:
  (1) one LLM decode step with the token drawn on the device, as the host loop runs it - the host's exponential draws (batchloop.draw_q), their
      upload and graph "AS" (the warpers in its key), against graph "Ar" alone (sampler row and seed read on the device, the draws formed in the
      tail) - for one dialogue (Engine.step_decode) and for an 8-row batch (RowBatch of 4: decode_begin + decode_end).  Wall time per step over
      `steps` steps from position 64 on, the token awaited every step as generate() awaits it; p50 (min - max) over the repetitions.
  (2) an 8-slot serving session with sampling on, 16 dialogues with the headline prompt and forced all-speech_diffusion schedules of 24..69 frames
      (random weights do not sample long speech runs): one session sampler against per-request samplers - four different rows, one of them
      greedy - in a session opened with seeded_tokens=True.  A forced token needs no draw, so the unseeded session's steps run the plain graph "A"
      here and the seeded session's run "Ar": the seeded leg is measured against the cheapest step there is.  Aggregate audio seconds per wall
      second, p50 (min - max).
Writes nothing itself: profiles/token_seed.txt holds a recorded run.
    python tools/mb_token_seed.py [repetitions=7] [steps=200]"""
import sys
import time
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
import bench
from vibevoice_rocm_amd import batchloop
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.rowbatch import RowBatch
from vibevoice_rocm_amd.synth import synth_state_dict_torch

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(20)
V = cfg.vocab
ST, SE, SD, EOS = V - 4, V - 3, V - 2, V - 1
valid = [ST, SE, SD, EOS]
ROW = (0.95, 0, 0.95)
fmt = lambda v: f"{sorted(v)[len(v) // 2]:.2f} ({min(v):.2f} - {max(v):.2f})"      # noqa: E731


def timed_steps(reset, step):
    reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / steps


# ---- (1) one dialogue
eng = m.engine
with torch.cuda.stream(eng.stream):
    eng.begin_sequence(64 + steps + 72, valid)
    eng.set_sampler(*ROW)
    eng.set_sampler_row(0, *ROW)


def reset_eng(seeded):
    def f():
        with torch.cuda.stream(eng.stream):
            eng.lens.fill_(64)
            if seeded:
                eng.set_token_seeds([1234])
            else:
                eng._seeded = False
    return f


legs = {"AS (host q + upload)": (reset_eng(False), lambda: eng.step_decode(ST, SD, None, q=batchloop.draw_q(4))),
        "Ar (seeded)": (reset_eng(True), lambda: eng.step_decode(ST, SD, None))}
res = {k: [] for k in legs}
for rep in range(reps + 1):
    for k, (reset, step) in legs.items():
        v = timed_steps(reset, step)
        if rep:
            res[k].append(v)
print("one dialogue, us per decode step p50 (min - max) of %d: " % reps + ";  ".join(f"{k}: {fmt(v)}" for k, v in res.items()), flush=True)

# ---- (1) 8-row batch
rb = RowBatch([m._lane(b) for b in range(4)], stream=eng.stream)
with torch.cuda.stream(eng.stream):
    rb.begin(64 + steps + 72, valid, 1.3)
    rb.set_sampler(*ROW)
    for b in range(4):
        rb.set_sampler_row(b, *ROW)
none = {b: None for b in range(4)}


def reset_rb(seeded):
    def f():
        with torch.cuda.stream(eng.stream):
            rb.lens.fill_(64)
            if seeded:
                rb.set_token_seeds([1234 + b for b in range(4)])
            else:
                rb._seeded = False
    return f


def step_rb(seeded):
    def f():
        rb.decode_begin(ST, SD, none, q=None if seeded else {b: batchloop.draw_q(4) for b in range(4)})
        rb.decode_end()
    return f


legs = {"AS (host q + upload)": (reset_rb(False), step_rb(False)), "Ar (seeded)": (reset_rb(True), step_rb(True))}
res = {k: [] for k in legs}
for rep in range(reps + 1):
    for k, (reset, step) in legs.items():
        v = timed_steps(reset, step)
        if rep:
            res[k].append(v)
print("8-row batch (4 dialogues), us per decode step p50 (min - max) of %d: " % reps + ";  ".join(f"{k}: {fmt(v)}" for k, v in res.items()), flush=True)
rb.close()
m.release_lanes()

# ---- (2) a session with sampling on
N, slots = 16, 8
frames = [24 + 3 * i for i in range(N)]
wls = [bench.build_workload(cfg, frames[i], 203, seed=301 + i) for i in range(N)]
tok = wls[0]["tok"]
L0 = wls[0]["input_ids"].shape[1]
mlt = max(2, -(-(max(frames) + 2) // L0) + 1)
GEN = {"do_sample": True, "temperature": 0.95, "top_p": 0.95}
MIXED = [GEN, {"do_sample": True, "temperature": 0.7, "top_k": 3}, {"do_sample": False}, {"do_sample": True, "temperature": 1.2, "top_p": 0.5}]


def leg_session(seeded):
    kw = dict(seeded_tokens=True) if seeded else dict(device_sampling=True)
    with m.open_session(tokenizer=tok, slots=slots, max_context=L0 + max(frames) + 2 + 8 + 64, generation_config=GEN, **kw) as sess:
        hs = []
        for i, w in enumerate(wls):
            per = dict(generation_config=MIXED[i % 4], token_seed=7000 + i) if seeded else {}
            hs.append(sess.submit(input_ids=w["input_ids"], cfg_scale=2.0, forced_tokens=w["forced"], speech_tensors=w["speech_tensors"].to(m.device),
                                  speech_masks=w["speech_masks"], speech_input_mask=w["speech_input_mask"], speech_noise=w["speech_noise"],
                                  max_length_times=mlt, max_new_tokens=len(w["forced"]), noise_seed=4000 + i, **per))
        sess.run()
    return sum(h.result().speech_outputs[0].shape[-1] for h in hs)


res = {False: [], True: []}
for rep in range(min(reps, 5) + 1):
    for seeded in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = leg_session(seeded)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert n == sum(frames) * cfg.hop, (n, sum(frames))
        if rep:
            res[seeded].append(n / 24000.0 / dt)
print(f"8-slot session, {N} dialogues of {min(frames)}..{max(frames)} frames, sampling on, aggregate audio-sec/s p50 (min - max) of {len(res[True])}: "
      f"one session sampler (forced tokens: graph A): {fmt(res[False])};  mixed per-request samplers, seeded (Ar): {fmt(res[True])}", flush=True)
