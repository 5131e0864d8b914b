"""LLM decode step (graph A: batch-2 Qwen2 step + tail) on a bf16 and on an fp8 (e4m3) KV cache, in one process on shared weights, as hipGraph
replays timed with device events; and vv_kv_quantize of a 400-token prompt.  python tools/mb_kv_fp8.py [1.5b|7b]   (profiles/kv_fp8.txt)"""
import ctypes as C
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from vibevoice_rocm_amd import _lib as L
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.engine import Engine
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch

model = sys.argv[1] if len(sys.argv) > 1 else "1.5b"
WARM, REPS = 10, 50
cfg = VVConfig.preset(model)
sd = synth_state_dict_torch(cfg, 1234, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(20)
e16 = m.engine
e8 = Engine(cfg, None, device="cuda:0", dtype=torch.bfloat16, weights_from=e16, kv_cache_dtype="fp8")
lib, V = e16.lib, cfg.vocab
SWEEP = {"1.5b": ((450, 1024), (1800, 2048), (3600, 4096), (7200, 8192), (16000, 16384), (32000, 32768), (64000, 65536)),
         "7b": ((450, 1024), (3600, 4096), (32000, 32768))}[model]


def events_ms(eng, fn, after=None):
    """median / min over REPS of the device time of fn() on the engine's stream (WARM untimed runs first)"""
    ts = []
    with torch.cuda.stream(eng.stream):
        for i in range(WARM + REPS):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(eng.stream)
            fn()
            b.record(eng.stream)
            if after is not None:
                after()
            if i >= WARM:
                ts.append((a, b))
    eng.stream.synchronize()
    ms = [a.elapsed_time(b) for a, b in ts]
    return statistics.median(ms), min(ms)


def step_ms(eng, S, smax):
    eng.begin_sequence(smax, [V - 4, V - 3, V - 2, V - 1])
    with torch.cuda.stream(eng.stream):
        eng.lens.copy_(torch.tensor([S, S // 3], dtype=torch.int32))
        lens0 = eng.lens.clone()
        L.check(lib.vv_graph_begin(eng.sp), "begin")
        eng._seq_A(V - 4, V - 2)
        ge = C.c_void_p()
        L.check(lib.vv_graph_end(eng.sp, C.byref(ge)), "end")
    r = events_ms(eng, lambda: L.check(lib.vv_graph_launch(ge, eng.sp), "launch"), lambda: eng.lens.copy_(lens0))
    lib.vv_graph_destroy(ge)
    return r


print(f"# {model}: LLM decode step (graph A), bf16 vs fp8 KV cache, median (min) of {REPS} graph replays after {WARM} warm-up, device events; "
      f"{torch.cuda.get_device_name(0)}", flush=True)
rows = []
for S, smax in SWEEP:
    b, f = step_ms(e16, S, smax), step_ms(e8, S, smax)
    rows.append((S, b[0], f[0]))
    print(f"{model} S={S} s_max={smax}: bf16 KV {b[0]:.3f} ({b[1]:.3f}) ms, fp8 KV {f[0]:.3f} ({f[1]:.3f}) ms, fp8 / bf16 = {f[0] / b[0]:.3f}", flush=True)
cross = next((S for S, b, f in rows if f < b), None)
print(f"{model}: first measured context at which the fp8-KV step is faster than the bf16-KV step: S = {cross}", flush=True)
base = rows[0]
for S, b, f in rows[1:]:
    if b > base[1]:
        print(f"{model} S={S}: context growth costs bf16 {b - base[1]:.3f} ms over S={base[0]}; fp8 KV recovers {b - f:.3f} ms = {(b - f) / (b - base[1]) * 100:.0f}% of it",
              flush=True)
# vv_kv_quantize of a 400-token prompt: row 0 with the scales, row 1 (one token) under them - the two calls prefill() makes
e8.begin_sequence(1024, [V - 4, V - 3, V - 2, V - 1])
with torch.cuda.stream(e8.stream):
    kv, t = e8._staging_kv(400)
    t[0].normal_()
    t[1].normal_()


def quant():
    L.check(lib.vv_kv_quantize(C.byref(kv), C.byref(e8.kv), 0, 0, 400, L.KVQ_DERIVE_SCALES, e8.sp), "quantize")
    L.check(lib.vv_kv_quantize(C.byref(kv), C.byref(e8.kv), 1, 1, 1, 0, e8.sp), "quantize")


q = events_ms(e8, quant)
print(f"{model}: vv_kv_quantize of a 400-token prompt (rows 0 and 1, {cfg.layers} layers x {cfg.kv_heads} KV heads): {q[0] * 1e3:.1f} ({q[1] * 1e3:.1f}) us", flush=True)
