"""generate() on 4 and 8 dialogues of the headline shape set up as the reference's application sets it up: the sde-dpmsolver++ scheduler
(main.py:543-548) and do_sample with temperature / top_p (main.py:1187-1196), no injected noise - row-batched (rowbatch.py) against the lanes,
alternating in one process after a warm-up call of each.  Prints audio-sec/s per call and the medians.

The token schedule stays forced (random weights would sample an end of speech within a few frames), so no token is drawn; the row-batched loop
still runs its sampling form (graph A1, one read-back of the logits, A2, no speculation) on every step, while a lane with a forced token takes its
one-graph step - the lanes' number is the optimistic one.  Every noise row (initial and the 20 per-step variance rows) is drawn on the host.
    python tools/mb_rowbatch_sde.py [frames=120] [batches=4,8] [timed calls per path=3]"""
import sys, time, types
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
import bench
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 120
batches = [int(v) for v in (sys.argv[2].split(",") if len(sys.argv) > 2 else ("4", "8"))]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.model.noise_scheduler = m.model.noise_scheduler.from_config(m.model.noise_scheduler.config, algorithm_type="sde-dpmsolver++",
                                                              beta_schedule="squaredcos_cap_v2")
m.set_ddpm_inference_steps(20)
assert m.engine.sde
args = types.SimpleNamespace(frames=frames, voice_frames=203, cfg_scale=2.0)
for batch in batches:
    wls = [bench.build_workload(cfg, frames, args.voice_frames, seed=201 + i) for i in range(batch)]
    ids = torch.cat([w["input_ids"] for w in wls])
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=wls[0]["tok"], cfg_scale=args.cfg_scale,
              forced_tokens=[w["forced"] for w in wls], speech_tensors=torch.cat([w["speech_tensors"] for w in wls]).cuda(),
              speech_masks=torch.cat([w["speech_masks"] for w in wls]), speech_input_mask=torch.cat([w["speech_input_mask"] for w in wls]),
              speech_noise=(torch.cat([w["speech_noise"][0] for w in wls]), torch.cat([w["speech_noise"][1] for w in wls])),
              generation_config={"do_sample": True, "temperature": 1.0, "top_p": 0.95}, show_progress_bar=False,
              max_length_times=max(2, -(-len(wls[0]["forced"]) // ids.shape[1]) + 1))
    rates = {False: [], True: []}
    m.release_lanes()                       # no row batch of an earlier size left over: the check below sees this size's
    for i in range(reps + 1):               # call 0 of each path warms up (lanes, row batches, graph captures)
        for rb in (False, True):
            torch.manual_seed(7)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = m.generate(row_batch=rb, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n = sum(o.shape[-1] for o in out.speech_outputs)
            assert n == batch * frames * cfg.hop, (n, batch, frames)
            assert not rb or m._rowbatch, "the row-batched path was not taken"
            if i:
                rates[rb].append(n / 24000.0 / dt)
    med = {rb: sorted(r)[len(r) // 2] for rb, r in rates.items()}
    print(f"batch {batch}, SDE + do_sample: lanes {med[False]:.1f} audio-sec/s (runs {', '.join(f'{v:.1f}' for v in rates[False])}), "
          f"row-batched {med[True]:.1f} (runs {', '.join(f'{v:.1f}' for v in rates[True])})", flush=True)
