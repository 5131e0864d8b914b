"""do_sample on the host sampler against device_sampling=True, 1.5B shapes, ODE solver, the application's sampling defaults (temperature 0.95,
top_p 0.95), NOTHING forced and nothing injected: a single dialogue, 4 dialogues row-batched and 4 on the lanes.  The legs alternate in one
process (host, device, host, device after a warm-up call of each), every call seeded alike, so both legs of a configuration sample the same
tokens and draw the same noise.

Random weights sample an end of speech within a few steps, so one call is short: each timed leg is `calls` seeded calls (seeds 0, 1, ...) and
the figure is the time per sampled LLM step over all of them, net of each call's prompt phase (a max_new_tokens=1 call of the same prompt, timed
the same way) - the cost the sampler path adds or removes sits in exactly those steps.  Frames per step are printed next to it.
    python tools/mb_sampling.py [calls per leg=24] [max_new_tokens=48]"""
import sys, time
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 24
max_new = int(sys.argv[2]) if len(sys.argv) > 2 else 48
cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(20)
V = cfg.vocab


class Tok:
    speech_start_id, speech_end_id, speech_diffusion_id, eos_token_id, bos_token_id, pad_id = V - 4, V - 3, V - 2, V - 1, None, 0


gen_cfg = {"do_sample": True, "temperature": 0.95, "top_p": 0.95}
g = torch.Generator().manual_seed(11)


def leg(ids, dev, rb, n_new, seeds):
    """(seconds, sampled steps, frames) over the seeded calls"""
    t, steps, frames = 0.0, 0, 0
    for s in seeds:
        torch.manual_seed(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = m.generate(input_ids=ids, tokenizer=Tok, cfg_scale=1.3, generation_config=gen_cfg, max_new_tokens=n_new, device_sampling=dev, row_batch=rb)
        torch.cuda.synchronize()
        t += time.perf_counter() - t0
        new = out.sequences[:, ids.shape[1]:]
        steps += int((new != Tok.pad_id).sum())
        frames += sum(0 if o is None else o.shape[-1] // cfg.hop for o in out.speech_outputs)
    return t, steps, frames


for name, B, rb in (("single dialogue", 1, False), ("4 dialogues row-batched", 4, True), ("4 dialogues on the lanes", 4, False)):
    ids = torch.cat([torch.randint(0, V - 8, (B, 63), generator=g), torch.full((B, 1), Tok.speech_start_id)], dim=1)
    m.release_lanes()
    res = {False: [], True: []}
    for rep in range(3):                      # rep 0 warms up (lanes, row batches, graph captures of both forms of graph A)
        for dev in (False, True):
            seeds = range(calls) if rep else range(2)
            t1, s1, _ = leg(ids, dev, rb, 1, seeds)
            t, s, f = leg(ids, dev, rb, max_new, seeds)
            if rep:
                res[dev].append((1e3 * (t - t1) / max(s - s1, 1), s - s1, f))
    line = []
    for dev in (False, True):
        line.append(f"{'device_sampling' if dev else 'host sampler'} " + " / ".join(f"{ms:.3f}" for ms, _, _ in res[dev]) + " ms per sampled step")
    assert res[False][0][1:] == res[True][0][1:], "the two legs did not sample the same tokens"
    print(f"{name}: {line[0]}; {line[1]}  ({res[True][0][1]} steps after the first token, {res[True][0][2]} frames per leg)", flush=True)
