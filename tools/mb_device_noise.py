"""device_noise=True against the host's noise draws, 1.5B shapes, bf16, ODE solver, 20 solver steps, a forced all-speech_diffusion schedule of the
headline shape (bench.build_workload: one voice of 203 frames, 88 text tokens, `frames` frames) - random weights do not sample long speech runs.
  (a) 4 and 8 dialogues row-batched in one generate() call: noise drawn on the host (noise=None: what a caller of the reference API gets, no
      frame is speculated), noise drawn on the device (device_noise=True), and - for scale - noise injected (noise=: the bench leg's form)
  (b) one dialogue, the headline workload: injected, drawn on the host, drawn on the device
The legs of a configuration alternate in one process after a warm-up call of each; the figure is audio seconds per wall second of the whole
call (voice encode and prefill included), p50 (min - max) over the repetitions.
    python tools/mb_device_noise.py [repetitions=5] [frames=225]"""
import sys, time
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
import bench
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 225
cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(20)


def call_kw(B):
    wls = [bench.build_workload(cfg, frames, 203, seed=201 + i) for i in range(B)]
    ids = torch.cat([w["input_ids"] for w in wls])
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=wls[0]["tok"], cfg_scale=1.3, forced_tokens=[w["forced"] for w in wls] if B > 1 else wls[0]["forced"],
              speech_tensors=torch.cat([w["speech_tensors"] for w in wls]).to(m.device), speech_masks=torch.cat([w["speech_masks"] for w in wls]),
              speech_input_mask=torch.cat([w["speech_input_mask"] for w in wls]),
              speech_noise=(torch.cat([w["speech_noise"][0] for w in wls]), torch.cat([w["speech_noise"][1] for w in wls])),
              generation_config={"do_sample": False}, max_length_times=max(2, -(-len(wls[0]["forced"]) // ids.shape[1]) + 1))
    noise = torch.stack([w["noise"] for w in wls]) if B > 1 else wls[0]["noise"]
    return kw, noise


def run(kw, leg, noise, B):
    extra = dict(injected=dict(noise=noise), host=dict(), device=dict(device_noise=True, noise_seed=list(range(1000, 1000 + B))))[leg]
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.generate(**kw, **extra)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    n = sum(o.shape[-1] for o in out.speech_outputs)
    assert n == B * frames * cfg.hop, (n, B, frames)
    return n / 24000.0 / dt


for B in (4, 8, 1):
    kw, noise = call_kw(B)
    if B > 1:
        kw["row_batch"] = True
    legs = ("host", "device", "injected")
    res = {k: [] for k in legs}
    for rep in range(reps + 1):                 # rep 0 warms up: lanes, row batches, the graph captures of both forms of graph B / H
        for leg in legs:
            v = run(kw, leg, noise, B)
            if rep:
                res[leg].append(v)
    name = f"{B} dialogues row-batched" if B > 1 else "one dialogue (headline workload)"
    fmt = lambda v: f"{sorted(v)[len(v) // 2]:.2f} ({min(v):.2f} - {max(v):.2f})"      # noqa: E731
    print(f"{name}, {frames} frames each, audio-sec/s p50 (min - max) of {reps}: noise drawn on the host {fmt(res['host'])};  device_noise {fmt(res['device'])};  "
          f"noise injected {fmt(res['injected'])}", flush=True)
    m.release_lanes()
