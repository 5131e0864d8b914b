"""A serving session against batched generate() on a ragged workload: 1.5B shapes, bf16, guidance 2.0, 20 solver steps, ODE solver, device noise,
24 dialogues with the headline prompt (bench.build_workload: one voice of 203 frames, 88 text tokens) and forced all-speech_diffusion schedules
whose frame counts are a fixed list spread evenly over 60..225, in a fixed shuffled arrival order - random weights do not sample long speech runs.
  (a) generate() on arrival-order batches of 8 (three calls, each as long as its longest dialogue)
  (b) one 8-slot session with all 24 submitted up front (a finished dialogue's slot goes to the next in the queue)
The legs alternate in one process after a warm-up pass of each; the figure is aggregate audio seconds per wall second of the whole leg (voice
encodes and prefills included), p50 (min - max) over the repetitions, next to the workload's own ceiling: of the row-steps leg (a) pays,
sum(len) / (8 * sum over batches of the batch's longest) do useful work, and a session can at best win the inverse of that.  Also printed:
the mean admission stall (host time of admit + prefill + first token, during which the running dialogues wait).
    python tools/mb_session.py [repetitions=5] [dialogues=24] [slots=8]"""
import random
import sys
import time
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
import bench
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 24
slots = int(sys.argv[3]) if len(sys.argv) > 3 else 8
CFG = 2.0
frames = [60 + round(i * 165 / max(N - 1, 1)) for i in range(N)]
random.Random(7).shuffle(frames)

cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(20)
wls = [bench.build_workload(cfg, frames[i], 203, seed=301 + i) for i in range(N)]
tok = wls[0]["tok"]
L0 = wls[0]["input_ids"].shape[1]
mlt = max(2, -(-(max(frames) + 2) // L0) + 1)
seeds = list(range(4000, 4000 + N))
batches = [list(range(i, min(i + slots, N))) for i in range(0, N, slots)]
useful = sum(frames) / (slots * sum(max(frames[i] for i in b) for b in batches))


def leg_generate():
    n = 0
    for b in batches:
        w = [wls[i] for i in b]
        ids = torch.cat([x["input_ids"] for x in w])
        out = m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=tok, cfg_scale=CFG, forced_tokens=[x["forced"] for x in w],
                         speech_tensors=torch.cat([x["speech_tensors"] for x in w]).to(m.device), speech_masks=torch.cat([x["speech_masks"] for x in w]),
                         speech_input_mask=torch.cat([x["speech_input_mask"] for x in w]),
                         speech_noise=(torch.cat([x["speech_noise"][0] for x in w]), torch.cat([x["speech_noise"][1] for x in w])),
                         generation_config={"do_sample": False}, max_length_times=mlt, max_new_tokens=max(len(x["forced"]) for x in w), row_batch=True, device_noise=True, noise_seed=[seeds[i] for i in b])
        n += sum(o.shape[-1] for o in out.speech_outputs)
    return n, None


def leg_session():
    with m.open_session(tokenizer=tok, slots=slots, max_context=L0 + max(frames) + 2 + 8 + 64) as sess:
        hs = [sess.submit(input_ids=w["input_ids"], cfg_scale=CFG, forced_tokens=w["forced"], speech_tensors=w["speech_tensors"].to(m.device),
                          speech_masks=w["speech_masks"], speech_input_mask=w["speech_input_mask"], speech_noise=w["speech_noise"],
                          max_length_times=mlt, max_new_tokens=len(w["forced"]), noise_seed=seeds[i]) for i, w in enumerate(wls)]
        sess.run()
        stall = list(sess.admission_ms)
    return sum(h.result().speech_outputs[0].shape[-1] for h in hs), stall


def timed(leg):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n, stall = leg()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    assert n == sum(frames) * cfg.hop, (n, sum(frames))
    return n / 24000.0 / dt, stall


legs = dict(generate=leg_generate, session=leg_session)
res, stalls = {k: [] for k in legs}, []
for rep in range(reps + 1):                         # rep 0 warms up: lanes, row batches, the graph captures of both legs
    for name, leg in legs.items():
        v, stall = timed(leg)
        if rep:
            res[name].append(v)
            if stall:
                stalls.append(sum(stall[slots:]) / max(1, len(stall[slots:])))       # the admissions into a running session
fmt = lambda v: f"{sorted(v)[len(v) // 2]:.2f} ({min(v):.2f} - {max(v):.2f})"      # noqa: E731
p50 = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
print(f"{N} dialogues, frames {min(frames)}..{max(frames)} (sum {sum(frames)}), arrival order {frames}", flush=True)
print(f"aggregate audio-sec/s p50 (min - max) of {reps}: (a) generate() in arrival-order batches of {slots}: {fmt(res['generate'])};  "
      f"(b) one {slots}-slot session: {fmt(res['session'])}", flush=True)
print(f"gain (b) / (a) at p50: {p50['session'] / p50['generate']:.3f};  workload ceiling: useful row-steps of (a) {useful:.3f} -> at most {1 / useful:.3f}", flush=True)
print(f"mean admission stall (admit + prefill + first token, mid-flight admissions): {sum(stalls) / max(1, len(stalls)):.2f} ms", flush=True)
