"""Weight-only MXFP6 e2m3 (weight_quant="mxfp6") against bf16, fp8 and mxfp4 on the batch-1/2 decode path; writes profiles/mxfp6_gemv.txt.

  1. per-launch us of the m = 2 GEMV on every per-frame matrix of 1.5B and 7B (the 14 matrices of profiles/mxfp4_gemv.txt), bf16 / fp8 / mxfp6 /
     mxfp4 in one process: per form a dependent hipGraph chain of vv_linear launches over enough weight copies that nothing is served from the
     caches, timed with device events; the four chains are built first and then timed in alternation, `rounds` rounds, and the figure is the
     p50 (min - max) over the rounds.  TB/s counts the bytes each form reads: bf16 2 B / weight, fp8 1 B + a row scale, mxfp6 0.75 B + 1 B per
     32 weights, mxfp4 0.5 B + 1 B per 32 weights;
  2. generate() per preset (1.5B, 7B), 1 dialogue, forced bench schedule (`frames` speech frames), injected noise, 20 steps: the four models
     are built side by side, warmed, and timed in alternation, `runs` >= 5 runs each (host clock around a call that ends in a device
     synchronise); audio-sec/s as p50 (min - max), and each quantised waveform's relative RMS against the bf16 one of the same process;
  3. (needs hipcc, no GPU) VGPRs, scratch, occupancy and LDS of every gemv_mx6_kernel from -Rpass-analysis=kernel-resource-usage.
    python tools/mb_mxfp6.py [sections=123] [frames=60] [runs=5] [presets=1.5b,7b] [out=profiles/mxfp6_gemv.txt] [rounds=5]
A section is appended to `out`; section 1 starts the file."""
import ctypes as C
import os
import re
import subprocess
import sys
import time

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)

argv = sys.argv[1:]
sections = argv[0] if len(argv) > 0 else "123"
frames = int(argv[1]) if len(argv) > 1 else 60
runs = max(5, int(argv[2])) if len(argv) > 2 else 5
presets = argv[3].split(",") if len(argv) > 3 else ["1.5b", "7b"]
out_path = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "mxfp6_gemv.txt")
rounds = int(argv[5]) if len(argv) > 5 else 5
FORMS = ("bf16", "fp8", "mxfp6", "mxfp4")
_out = open(out_path, "w" if "1" in sections else "a")


def say(line):
    print(line, flush=True)
    _out.write(line + "\n")
    _out.flush()


def p50(v):
    s = sorted(v)
    return s[len(s) // 2]


def section_3():
    from vibevoice_rocm_amd import build as vb
    src = os.path.join(vb.HERE, "csrc", "vv_gemv_mx6.hip")
    cmd = [vb.find_hipcc(), *vb.FLAGS, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(vb.HERE, "csrc"), "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    say("# 3. build checks of csrc/vv_gemv_mx6.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("# gemv_mx6_kernel<M, DUAL, KSPLIT, KU> instantiations: M DUAL KSPLIT KU | VGPRs scratch(B/lane) occupancy(waves/SIMD) LDS(B/block); LDS = the RMSNorm / split-K")
    say("# reduction slots only: the decode path has no table and no LDS")
    rows = []
    for blk in re.split(r"remark: [^\n]*Function Name: ", err)[1:]:
        m = re.match(r"\S*gemv_mx6_kernelILi(\d)ELb([01])ELi(\d+)ELi(\d)EE", blk)
        if not m:
            continue
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
        rows.append((tuple(int(v) for v in m.groups()), g("VGPRs"), g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]"), g("LDS Size [bytes/block]")))
    for (mm, dual, ks, ku), vg, sc, occ, lds in sorted(rows):
        say(f"  M={mm} dual={dual} ksplit={ks:2d} ku={ku} | vgpr {vg:3d} scratch {sc} occ {occ} lds {lds}")
    say(f"# {len(rows)} kernels, scratch {'0 in every one' if all(r[2] == 0 for r in rows) else 'NOT ZERO: ' + str([r[0] for r in rows if r[2]])}")
    assert rows and all(r[2] == 0 for r in rows)


if sections == "3":
    section_3()
    sys.exit(0)

import numpy as np
import torch
import bench
from vibevoice_rocm_amd import _lib as L
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch
from vibevoice_rocm_amd.weights import pack_mxfp4, pack_mxfp6, quantize_e4m3_pow2, quantize_mxfp4, quantize_mxfp6

if not torch.cuda.is_available():
    raise SystemExit("tools/mb_mxfp6.py: sections 1 and 2 measure on the GPU and there is none (no fallback)")
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
WDT = {"bf16": L.VV_BF16, "fp8": L.VV_FP8, "mxfp6": L.VV_MXFP6, "mxfp4": L.VV_MXFP4}


def _bytes(n, k, form):
    return {"bf16": 2 * n * k, "fp8": n * k + 4 * n, "mxfp6": 3 * n * k // 4 + n * k // 32, "mxfp4": n * k // 2 + n * k // 32}[form]


def _mat(w, form):
    if form == "bf16":
        return (w.bfloat16(), None)
    if form == "fp8":
        q, s, _ = quantize_e4m3_pow2(w)
        return (q, s)
    if form == "mxfp6":
        c, s, _ = quantize_mxfp6(w.bfloat16())
        return pack_mxfp6(c, s)
    c, s, _ = quantize_mxfp4(w.bfloat16())
    return pack_mxfp4(c, s)


class Chain:
    """N dependent vv_linear launches in one graph; the weights cycle through enough copies to exceed 1.2 GB"""

    def __init__(self, m, n, k, dual, form, pro=0, mod=False, epi=False, bias=False, gelu=False, flags=0, N=120):
        self.st, self.N = torch.cuda.Stream(), N
        self.per = _bytes(n, k, form) * (2 if dual else 1)
        copies = min(N, max(2, int(1.2e9 // self.per)))
        with torch.cuda.stream(self.st):
            ld = max(n, k)
            bufs = [torch.randn(m, ld, device="cuda") * 0.5 for _ in range(2)]
            base = [torch.randn(n, k, device="cuda") / k ** 0.5 for _j in range(2 if dual else 1)]
            ws = [[_mat(torch.roll(b, c, 0), form) for b in base] for c in range(copies)]
            nw = torch.ones(k, device="cuda")
            sh, sc = torch.zeros(m, k, device="cuda"), torch.zeros(m, k, device="cuda")
            gate, b = torch.full((m, n), 0.5, device="cuda"), torch.zeros(n, device="cuda")
            self.keep = (bufs, ws, nw, sh, sc, gate, b)
            args = []
            for i in range(N):
                a = L.LinArgs()
                a.x, a.ldx, a.m, a.n, a.k = bufs[i & 1].data_ptr(), ld, m, n, k
                a.out, a.ldo = bufs[(i + 1) & 1].data_ptr(), ld
                a.pro, a.norm_w, a.eps, a.flags = pro, (nw.data_ptr() if pro == 1 else 0), 1e-5, flags
                if mod:
                    a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
                mats = ws[i % copies]
                a.wdt = WDT[form]
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
            name = C.create_string_buffer(192)
            L.check(lib.vv_linear_route(C.byref(args[0]), name, 192), "vv_linear_route")
            self.route = name.value.decode()
            self.st.synchronize()
            L.check(lib.vv_graph_begin(self.st.cuda_stream), "graph begin")
            for a in args:
                L.check(lib.vv_linear(C.byref(a), self.st.cuda_stream), "vv_linear")
            self.ge = C.c_void_p()
            L.check(lib.vv_graph_end(self.st.cuda_stream, C.byref(self.ge)), "graph end")
            for _ in range(3):
                lib.vv_graph_launch(self.ge, self.st.cuda_stream)
            self.st.synchronize()

    def time_us(self, reps=5):
        with torch.cuda.stream(self.st):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(self.st)
            for _ in range(reps):
                lib.vv_graph_launch(self.ge, self.st.cuda_stream)
            e1.record(self.st)
            self.st.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps / self.N

    def close(self):
        lib.vv_graph_destroy(self.ge)
        self.keep = None


if "1" in sections:
    say(f"# tools/mb_mxfp6.py on one {torch.cuda.get_device_name(0)} (gfx950): weight-only MXFP6 (e2m3) vs fp8 vs MXFP4 vs bf16 on the batch-1/2 decode path.")
    say("# Synthetic random-init weights; generate() legs use the bench workload (1 dialogue, forced schedule, injected noise, 20 steps).")
    say(f"# 1. GEMV at m = 2, us per launch as p50 (min - max) over {rounds} alternating rounds (dependent graph chain of 120 launches x 5 per round, "
        "device events) and TB/s of the bytes each form reads at the p50")
    for name, n, k, dual, kw in SHAPES:
        chains = {f: Chain(2, n, k, dual, f, **kw) for f in FORMS}
        t = {f: [] for f in FORMS}
        for _ in range(rounds):
            for f in FORMS:
                t[f].append(chains[f].time_us())
        mid = {f: p50(t[f]) for f in FORMS}
        say(f"{name:18s} n={n:5d} k={k:5d}{' dual' if dual else '     '}  " +
            "  ".join(f"{f} {mid[f]:6.2f} ({min(t[f]):6.2f} - {max(t[f]):6.2f}) us {chains[f].per / mid[f] / 1e6:5.2f} TB/s" for f in FORMS) +
            f"   mxfp6/fp8 time {mid['mxfp6'] / mid['fp8']:.2f}  mxfp6/mxfp4 time {mid['mxfp6'] / mid['mxfp4']:.2f}   [{chains['mxfp6'].route}]")
        for c in chains.values():
            c.close()
        del chains
        torch.cuda.empty_cache()

if "2" in sections:
    say(f"# 2. generate(), 1 dialogue, {frames} forced speech frames, injected noise, 20 steps; audio-sec/s as p50 (min - max) over {runs} runs per mode, "
        "the four modes alternating; waveforms vs bf16 in the same process.")
    say("# The weights are synthetic: a waveform deviation here says how far the quantised arithmetic moves THIS random model's output, and nothing "
        "about a real checkpoint's audio quality.")
    for preset in presets:
        cfg = VVConfig.preset(preset)
        sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
        wl = bench.build_workload(cfg, frames, 203, seed=201)
        kw = dict(input_ids=wl["input_ids"], tokenizer=wl["tok"], cfg_scale=2.0, forced_tokens=wl["forced"],
                  speech_tensors=wl["speech_tensors"].cuda(), speech_masks=wl["speech_masks"], speech_input_mask=wl["speech_input_mask"],
                  speech_noise=wl["speech_noise"], noise=wl["noise"], show_progress_bar=False,
                  max_length_times=max(2, -(-len(wl["forced"]) // wl["input_ids"].shape[1]) + 1))
        models, outs, rates = {}, {}, {f: [] for f in FORMS}
        for f in FORMS:
            models[f] = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=None if f == "bf16" else f)
            models[f].set_ddpm_inference_steps(20)
        for i in range(runs + 1):                     # run 0 warms every mode
            for f in FORMS:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = models[f].generate(**kw)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                wav = out.speech_outputs[0].float().cpu().numpy().ravel()
                assert wav.size == frames * cfg.hop, (wav.size, frames)
                outs[f] = wav
                if i:
                    rates[f].append(wav.size / 24000.0 / dt)
        for f in FORMS:
            say(f"{preset} {f:5s}: {p50(rates[f]):6.2f} ({min(rates[f]):.2f} - {max(rates[f]):.2f}) audio-sec/s, device weights {models[f].engine.w.nbytes() / 1e9:.2f} GB")
        ref = outs["bf16"]
        for f in FORMS[1:]:
            e = float(np.sqrt(np.mean((outs[f] - ref) ** 2)) / max(np.sqrt(np.mean(ref ** 2)), 1e-30))
            ok = bool(np.isfinite(outs[f]).all()) and e < 1.0
            say(f"{preset} {f} vs bf16 waveform: rel RMS {e:.3e} {'(finite)' if ok else '(WRONG OUTPUT: speed figure void)'}; "
                f"speed vs bf16 {p50(rates[f]) / p50(rates['bf16']):.3f}")
        say(f"{preset} mxfp6 / fp8 speed {p50(rates['mxfp6']) / p50(rates['fp8']):.3f}   mxfp6 / mxfp4 speed {p50(rates['mxfp6']) / p50(rates['mxfp4']):.3f}")
        del models, sd
        torch.cuda.empty_cache()

if "3" in sections:
    section_3()
