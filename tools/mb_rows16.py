"""Wide row batches (row_batch_width=8, csrc gemv_rows16_kernel) against the default partition, one process, alternating legs, p50 (min - max):
  matrices   the six decode matrices of 1.5B in a dependent hipGraph chain (tools/mb_chain_lin.py): ONE 16-row launch on the fragment-major
             copy against TWO 8-row launches (us per 16 rows, bytes / s of one weight pass)
  generate   bench.batched_leg at 6, 8, 10, 12, 16 dialogues (225 frames, forced schedule, 1.5B bf16), row_batch_width 4 against 8: aggregate
             audio-sec/s; with VV_RB_TIMING=1 in the environment the row batches print their per-step A / H / tails times
  session    one 16-slot session with 32 dialogues of 60..225 frames submitted up front, width 4 against 8
    python tools/mb_rows16.py [matrices] [generate[=6,8,10,12,16]] [session] [reps=2]"""
import random
import statistics
import sys
import time
import types

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tools")
import torch

what = [a for a in sys.argv[1:] if not a.startswith("reps=")] or ["matrices", "generate", "session"]
reps = next((int(a[5:]) for a in sys.argv[1:] if a.startswith("reps=")), 2)


def p50(v):
    return f"{statistics.median(v):7.2f} ({min(v):.2f} - {max(v):.2f})"


if "matrices" in what:
    import contextlib
    import io
    import mb_chain_lin as M
    from mb_rows8 import SHAPES
    M.L.check(M.lib.vv_init(), "init")
    M.L.check(M.lib.vv_tune(b"gemv_rows_scratch", 1), "scratch")
    print("per matrix: us per pass over the weights for 16 rows, p50 (min - max) of 5 alternating rounds; GB/s of one weight pass at the p50")
    for name, a, kw in SHAPES:
        t16, t8 = [], []
        for _ in range(5):
            with contextlib.redirect_stdout(io.StringIO()):
                t16.append(M.chain(16, *a, frag=True, **kw))
                t8.append(2 * M.chain(8, *a, frag=True, **kw))
        n, k, dual = a[0], a[1], a[2]
        byts = n * k * 2 * (2 if dual else 1)
        print(f"  {name:<13} n={n:5d} k={k:5d}: one 16-row launch {p50(t16)} us ({byts / statistics.median(t16) / 1e3:5.0f} GB/s)   "
              f"two 8-row launches {p50(t8)} us ({2 * byts / statistics.median(t8) / 1e3:5.0f} GB/s)", flush=True)
    M.lib.vv_tune(b"gemv_rows_scratch", 0)

gen = next((a for a in what if a.startswith("generate")), None)
if gen or "session" in what:
    import bench
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset("1.5b")
    sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m.set_ddpm_inference_steps(20)

if gen:
    args = types.SimpleNamespace(frames=225, voice_frames=203, cfg_scale=2.0)
    batches = [int(v) for v in gen.split("=")[1].split(",")] if "=" in gen else [6, 8, 10, 12, 16]
    print(f"generate(): aggregate audio-sec/s, p50 (min - max) of {3 * reps} timed calls per leg (legs alternate; two warm-up calls in front of each three)")
    for B in batches:
        runs = {4: [], 8: []}
        for _ in range(reps):
            for w in (4, 8):
                m.row_batch_width = w
                runs[w] += bench.batched_leg(m, cfg, args, B, row_batch=True)["runs"]
        m.row_batch_width = 4
        print(f"  {B:2d} dialogues: width 4 {p50(runs[4])}   width 8 {p50(runs[8])}   ratio {statistics.median(runs[8]) / statistics.median(runs[4]):.3f}", flush=True)

if "session" in what:
    N, slots = 32, 16
    frames = [60 + round(i * 165 / (N - 1)) for i in range(N)]
    random.Random(7).shuffle(frames)
    wls = [bench.build_workload(cfg, frames[i], 203, seed=301 + i) for i in range(N)]
    tok, L0 = wls[0]["tok"], wls[0]["input_ids"].shape[1]
    runs = {4: [], 8: []}
    for r in range(reps + 1):              # the first round warms up (graphs, lanes) and is dropped
        for w in (4, 8):
            m.row_batch_width = w
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with m.open_session(tokenizer=tok, slots=slots, max_context=L0 + max(frames) + 2 + 8 + 64) as sess:
                hs = [sess.submit(input_ids=wl["input_ids"], cfg_scale=2.0, forced_tokens=wl["forced"], speech_tensors=wl["speech_tensors"].to(m.device),
                                  speech_masks=wl["speech_masks"], speech_input_mask=wl["speech_input_mask"], speech_noise=wl["speech_noise"],
                                  max_length_times=max(2, -(-(max(frames) + 2) // L0) + 1), max_new_tokens=len(wl["forced"]), noise_seed=4000 + i)
                      for i, wl in enumerate(wls)]
                sess.run()
                n = sum(h.result().speech_outputs[0].shape[-1] for h in hs)
            torch.cuda.synchronize()
            if r:
                runs[w].append(n / 24000.0 / (time.perf_counter() - t0))
    m.row_batch_width = 4
    print(f"session, {slots} slots, {N} dialogues of 60..225 frames: width 4 {p50(runs[4])}   width 8 {p50(runs[8])} audio-sec/s", flush=True)
