"""Weight-only NF4 (weight_quant="nf4") against bf16 and fp8 on the batch-1/2 decode path, one process:

  1. per-launch us of the streaming GEMV at m = 2 on every per-frame matrix of 1.5B and 7B, bf16 vs fp8 vs nf4 (a dependent hipGraph chain of
     vv_linear launches over enough weight copies that nothing is served from the caches, timed with device events; residual projections in
     place, as the composites call them).  TB/s counts the bytes each form reads: bf16 2 B / weight, fp8 1 B + a row scale, nf4 0.5 B + 4 B
     per 64 weights;
  2. generate() per preset (1.5B, 7B), 1 dialogue, forced bench schedule (`frames` speech frames), injected noise, 20 steps, bf16 / fp8 / nf4
     after a warm-up call of each; the fp8 and nf4 waveforms are compared with the bf16 one of the same run before their speed is printed.
    python tools/mb_nf4.py [frames=60] [timed calls per leg=2] [presets=1.5b,7b]"""
import ctypes as C
import sys
import time
import types

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import numpy as np
import torch
import bench
from vibevoice_rocm_amd import _lib as L
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch
from vibevoice_rocm_amd.weights import pack_nf4, quantize_e4m3_pow2, quantize_nf4

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 60
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 2
presets = sys.argv[3].split(",") if len(sys.argv) > 3 else ["1.5b", "7b"]
lib = L.load()
L.check(lib.vv_init(), "vv_init")

RB = dict(flags=L.LIN_W_REUSED)
SHAPES = (("1.5B llm qkv", 2048, 1536, False, dict(pro=1, bias=True)), ("1.5B llm o", 1536, 1536, False, dict(epi=True)),
          ("1.5B llm gate/up", 8960, 1536, True, dict(pro=1)), ("1.5B llm down", 1536, 8960, False, dict(epi=True)),
          ("1.5B head gate/up", 4608, 1536, True, dict(pro=1, mod=True, **RB)), ("1.5B head down", 1536, 4608, False, dict(epi=True, **RB)),
          ("conv ffn lin1", 8192, 2048, False, dict(pro=1, bias=True, gelu=True)), ("conv ffn lin2", 2048, 8192, False, dict(epi=True, bias=True)),
          ("7B llm qkv", 4608, 3584, False, dict(pro=1, bias=True)), ("7B llm o", 3584, 3584, False, dict(epi=True)),
          ("7B llm gate/up", 18944, 3584, True, dict(pro=1)), ("7B llm down", 3584, 18944, False, dict(epi=True)),
          ("7B head gate/up", 10752, 3584, True, dict(pro=1, mod=True, **RB)), ("7B head down", 3584, 10752, False, dict(epi=True, **RB)))


def _bytes(n, k, form):
    return {"bf16": 2 * n * k, "fp8": n * k + 4 * n, "nf4": n * k // 2 + 4 * n * k // 64}[form]


def _mat(w, form):
    if form == "bf16":
        return (w.bfloat16(), None)
    if form == "fp8":
        q, s, _ = quantize_e4m3_pow2(w)
        return (q, s)
    c, s, _ = quantize_nf4(w.bfloat16())
    return pack_nf4(c, s)


def chain_us(m, n, k, dual, form, pro=0, mod=False, epi=False, bias=False, gelu=False, flags=0, N=120):
    """mean us per launch of N dependent vv_linear launches in one graph; the weights cycle through enough copies to exceed 1.2 GB"""
    st = torch.cuda.Stream()
    per = _bytes(n, k, form) * (2 if dual else 1)
    copies = min(N, max(2, int(1.2e9 // per)))
    with torch.cuda.stream(st):
        ld = max(n, k)
        bufs = [torch.randn(m, ld, device="cuda") * 0.5 for _ in range(2)]
        ws = [[_mat(torch.randn(n, k, device="cuda") / k ** 0.5, form) for _j in range(2 if dual else 1)] for _ in range(copies)]
        nw = torch.ones(k, device="cuda")
        sh, sc = torch.zeros(m, k, device="cuda"), torch.zeros(m, k, device="cuda")
        gate, b = torch.full((m, n), 0.5, device="cuda"), torch.zeros(n, device="cuda")
        args = []
        for i in range(N):
            a = L.LinArgs()
            a.x, a.ldx, a.m, a.n, a.k = bufs[i & 1].data_ptr(), ld, m, n, k
            a.out, a.ldo = bufs[(i + 1) & 1].data_ptr(), ld
            a.pro, a.norm_w, a.eps, a.flags = pro, (nw.data_ptr() if pro == 1 else 0), 1e-5, flags
            if mod:
                a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
            mats = ws[i % copies]
            a.wdt = {"bf16": L.VV_BF16, "fp8": L.VV_FP8, "nf4": L.VV_NF4}[form]
            a.w, a.wscale = mats[0][0].data_ptr(), (mats[0][1].data_ptr() if mats[0][1] is not None else 0)
            if dual:
                a.w2, a.act = mats[1][0].data_ptr(), 2
                a.w2scale = mats[1][1].data_ptr() if mats[1][1] is not None else 0
            elif gelu:
                a.act = 1
            if epi:
                a.gate, a.gate_ld, a.res, a.ldres = gate.data_ptr(), n, a.out, ld
            if bias:
                a.bias = b.data_ptr()
            args.append(a)
        st.synchronize()
        L.check(lib.vv_graph_begin(st.cuda_stream), "graph begin")
        for a in args:
            L.check(lib.vv_linear(C.byref(a), st.cuda_stream), "vv_linear")
        ge = C.c_void_p()
        L.check(lib.vv_graph_end(st.cuda_stream, C.byref(ge)), "graph end")
        for _ in range(3):
            lib.vv_graph_launch(ge, st.cuda_stream)
        st.synchronize()
        best = 1e9
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(5):
                lib.vv_graph_launch(ge, st.cuda_stream)
            e1.record(st)
            st.synchronize()
            best = min(best, e0.elapsed_time(e1) * 1e3 / 5 / N)
        lib.vv_graph_destroy(ge)
    del ws
    torch.cuda.empty_cache()
    return best, per


print(f"# 1. streaming GEMV, m = 2, us per launch (dependent graph chain, device events) and TB/s of the bytes each form reads", flush=True)
for name, n, k, dual, kw in SHAPES:
    r = {f: chain_us(2, n, k, dual, f, **kw) for f in ("bf16", "fp8", "nf4")}
    print(f"{name:18s} n={n:5d} k={k:5d}{' dual' if dual else '     '}  " +
          "  ".join(f"{f} {t:7.2f} us {b / t / 1e6:5.2f} TB/s" for f, (t, b) in r.items()) +
          f"   nf4/fp8 {r['nf4'][0] / r['fp8'][0]:.2f}  fp8/nf4 speed-up {r['fp8'][0] / r['nf4'][0]:.2f}x", flush=True)

print(f"# 2. generate(), 1 dialogue, {frames} forced speech frames, injected noise, 20 steps; outputs vs bf16 in the same run", flush=True)
for preset in presets:
    cfg = VVConfig.preset(preset)
    sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
    wl = bench.build_workload(cfg, frames, 203, seed=201)
    kw = dict(input_ids=wl["input_ids"], tokenizer=wl["tok"], cfg_scale=2.0, forced_tokens=wl["forced"],
              speech_tensors=wl["speech_tensors"].cuda(), speech_masks=wl["speech_masks"], speech_input_mask=wl["speech_input_mask"],
              speech_noise=wl["speech_noise"], noise=wl["noise"], show_progress_bar=False,
              max_length_times=max(2, -(-len(wl["forced"]) // wl["input_ids"].shape[1]) + 1))
    outs, rates = {}, {}
    for q in (None, "fp8", "nf4"):
        mm = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=q)
        mm.set_ddpm_inference_steps(20)
        rr = []
        for i in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = mm.generate(**kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            wav = out.speech_outputs[0].float().cpu().numpy().ravel()
            assert wav.size == frames * cfg.hop, (wav.size, frames)
            if i:
                rr.append(wav.size / 24000.0 / dt)
        outs[q or "bf16"], rates[q or "bf16"] = wav, sorted(rr)[len(rr) // 2]
        mem = mm.engine.w.nbytes() / 1e9
        del mm
        torch.cuda.empty_cache()
        print(f"{preset} {q or 'bf16':4s}: {rates[q or 'bf16']:6.2f} audio-sec/s (runs {', '.join(f'{v:.2f}' for v in rr)}), device weights {mem:.2f} GB",
              flush=True)
    ref = outs["bf16"]
    for q in ("fp8", "nf4"):
        e = float(np.sqrt(np.mean((outs[q] - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))
        ok = bool(np.isfinite(outs[q]).all()) and e < 0.5
        print(f"{preset} {q} vs bf16 waveform: rel RMS {e:.3e} {'(ok)' if ok else '(WRONG OUTPUT: speed figure void)'}; "
              f"speed vs bf16 {rates[q] / rates['bf16']:.3f}", flush=True)
    print(f"{preset} nf4 / fp8 speed {rates['nf4'] / rates['fp8']:.3f}", flush=True)
    del sd
    torch.cuda.empty_cache()
