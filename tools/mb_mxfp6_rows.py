"""MXFP6 on the row-batched decode path (weight_quant="mxfp6", mxfp6_row_batch=True; csrc/vv_gemv_rows_mx6.hip) against the fp8, MXFP4 and bf16
forms of the 3..8-row matrix-core GEMV and against MXFP6 on the lanes; writes profiles/mxfp6_rows.txt.  After tools/mb_mxfp6.py and
tools/mb_mxfp4_rows.py (whose method this is).

  1. per-launch us of the m = 8 rows GEMV on the LLM and head matrices of 1.5B and 7B, fragment-major fp8 / mxfp4 / mxfp6 in one process: per
     form a dependent hipGraph chain of vv_linear launches (process-wide split-K scratch on) over enough weight copies that nothing is served
     from the caches, timed with device events; the chains are built first and then timed in alternation, `rounds` rounds; p50 (min - max).
     TB/s counts the bytes each form reads: fp8 1 B / weight + a row scale, mxfp4 0.5 B + 1 B per 32 weights, mxfp6 0.75 B + 1 B per 32;
  2. generate() on 4 and 8 dialogues per preset, forced bench schedule (`frames` speech frames), injected noise, 20 steps, in five modes built
     side by side and timed in alternation after a warm-up, `runs` >= 5 runs each (host clock around a call that ends in a device
     synchronise): mxfp6 on the lanes (mxfp6_row_batch off: the default), mxfp6 row-batched, fp8 row-batched, mxfp4 row-batched, bf16
     row-batched; aggregate audio-sec/s as p50 (min - max), device weight bytes, and the two mxfp6 waveforms against each other.  `rotate` turns
     the list of modes by that many places for the order the models are built in AND the order they are timed in (each model keeps its
     engines' HIP streams for the run): a figure that is the kernel's holds under every rotation.  A GAIN is counted only where the mxfp6 rows'
     minimum lies above the mxfp6 lanes' maximum;
  3. (needs hipcc, no GPU) VGPRs, scratch, occupancy and LDS of every kernel of csrc/vv_gemv_rows_mx6.hip from -Rpass-analysis=kernel-resource-usage.
    python tools/mb_mxfp6_rows.py [sections=123] [frames=60] [runs=5] [presets=1.5b,7b] [out=profiles/mxfp6_rows.txt] [rounds=5] [batches=4,8] [rotate=0]
A section is appended to `out`; section 1 starts the file."""
import ctypes as C
import gc
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
out_path = argv[4] if len(argv) > 4 else os.path.join(ROOT, "profiles", "mxfp6_rows.txt")
rounds = int(argv[5]) if len(argv) > 5 else 5
batches = [int(b) for b in argv[6].split(",")] if len(argv) > 6 else [4, 8]
rotate = int(argv[7]) if len(argv) > 7 else 0
FORMS = ("fp8", "mxfp4", "mxfp6")
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
    src = os.path.join(vb.HERE, "csrc", "vv_gemv_rows_mx6.hip")
    cmd = [vb.find_hipcc(), *vb.FLAGS, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(vb.HERE, "csrc"), "--cuda-device-only", "-S",
           "-Rpass-analysis=kernel-resource-usage", src, "-o", os.devnull]
    err = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    say("# 3. build checks of csrc/vv_gemv_rows_mx6.hip (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage)")
    say("# gemv_rows_mx6_kernel<DUAL, NW, KS, PERS> instantiations: DUAL NW KS PERS | VGPRs scratch(B/lane) occupancy(waves/SIMD) static LDS(B/block) + dynamic LDS (the A fragments)")
    rows = []
    for blk in re.split(r"remark: [^\n]*Function Name: ", err)[1:]:
        m = re.match(r"\S*gemv_rows_mx6_kernelILb([01])ELi(\d)ELi(\d)ELb([01])E", blk)
        if not m:
            continue
        g = lambda key: int(re.search(re.escape(key) + r": (\d+)", blk).group(1))
        rows.append((tuple(int(v) for v in m.groups()), g("VGPRs"), g("ScratchSize [bytes/lane]"), g("Occupancy [waves/SIMD]"), g("LDS Size [bytes/block]")))
    for (dual, nw, ks, pers), vg, sc, occ, lds in sorted(rows):
        say(f"  dual={dual} nw={nw} ks={ks} pers={pers} | vgpr {vg:3d} scratch {sc} occ {occ} lds {lds:5d} + {nw * 4 * ks * 1024:5d}")
    say(f"# {len(rows)} kernels, scratch {'0 in every one' if all(r[2] == 0 for r in rows) else 'NOT ZERO: ' + str([r[0] for r in rows if r[2]])}")
    assert len(rows) == 10 and all(r[2] == 0 for r in rows)


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
from vibevoice_rocm_amd.weights import DeviceWeights, quantize_e4m3_pow2, quantize_mxfp4, quantize_mxfp6

if not torch.cuda.is_available():
    raise SystemExit("tools/mb_mxfp6_rows.py: sections 1 and 2 measure on the GPU and there is none (no fallback)")
lib = L.load()
L.check(lib.vv_init(), "vv_init")

RB = dict(flags=L.LIN_W_REUSED)
SHAPES = (("1.5B llm qkv", 2048, 1536, False, dict(pro=1, bias=True)), ("1.5B llm o", 1536, 1536, False, dict(epi=True)),
          ("1.5B llm gate/up", 8960, 1536, True, dict(pro=1)), ("1.5B llm down", 1536, 8960, False, dict(epi=True)),
          ("1.5B head gate/up", 4608, 1536, True, dict(pro=1, mod=True, **RB)), ("1.5B head down", 1536, 4608, False, dict(epi=True, **RB)),
          ("7B llm qkv", 4608, 3584, False, dict(pro=1, bias=True)), ("7B llm o", 3584, 3584, False, dict(epi=True)),
          ("7B llm gate/up", 18944, 3584, True, dict(pro=1)), ("7B llm down", 3584, 18944, False, dict(epi=True)),
          ("7B head gate/up", 10752, 3584, True, dict(pro=1, mod=True, **RB)), ("7B head down", 3584, 10752, False, dict(epi=True, **RB)))
WDT = {"bf16": L.VV_BF16, "fp8": L.VV_FP8, "mxfp4": L.VV_MXFP4_FRAG, "mxfp6": L.VV_MXFP6_FRAG}
SCALE_OFF = {"mxfp4": 2, "mxfp6": 3}      # the scale bytes sit behind the codes: n k / 2, n k 3 / 4


def _bytes(n, k, form):
    return {"bf16": 2 * n * k, "fp8": n * k + 4 * n, "mxfp4": n * k // 2 + n * k // 32, "mxfp6": n * k * 3 // 4 + n * k // 32}[form]


def _mat(w, form):
    """(fragment-major weights, scale pointer source or None)"""
    if form == "bf16":
        return (DeviceWeights.frag_major(w.bfloat16()), None)
    if form == "fp8":
        q, s, _ = quantize_e4m3_pow2(w)
        return (DeviceWeights.frag_major_fp8(q), s)
    if form == "mxfp6":
        c, s, _ = quantize_mxfp6(w.bfloat16())
        return (DeviceWeights.frag_major_mxfp6(c, s), "tail")
    c, s, _ = quantize_mxfp4(w.bfloat16())
    return (DeviceWeights.frag_major_mxfp4(c, s), "tail")


class Chain:
    """N dependent vv_linear launches at m rows in one graph; the weights cycle through enough copies to exceed 1.2 GB.  None: the form does not
    cover the call (the adaLN prologue beyond K = 2048: the engine runs those on the row-major bf16 matrices)"""

    def __init__(self, m, n, k, dual, form, pro=0, mod=False, epi=False, bias=False, flags=0, N=120):
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
                a.pro, a.norm_w, a.eps, a.flags = pro, (nw.data_ptr() if pro == 1 else 0), 1e-5, flags | L.LIN_W_FRAG
                if mod:
                    a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
                mats = ws[i % copies]
                a.wdt = WDT[form]

                def scale_of(mt):
                    return 0 if mt[1] is None else (mt[0].data_ptr() + n * k * SCALE_OFF[form] // 4 if isinstance(mt[1], str) else mt[1].data_ptr())
                a.w, a.wscale = mats[0][0].data_ptr(), scale_of(mats[0])
                if dual:
                    a.w2, a.act, a.w2scale = mats[1][0].data_ptr(), 2, scale_of(mats[1])
                if epi:
                    a.gate, a.gate_ld, a.res, a.ldres = gate.data_ptr(), n, a.out, ld
                if bias:
                    a.bias = b.data_ptr()
                args.append(a)
            name = C.create_string_buffer(192)
            self.route = None
            if lib.vv_linear_route(C.byref(args[0]), name, 192) != 0:
                return
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
        if self.route is not None:
            lib.vv_graph_destroy(self.ge)
        self.keep = None


if "1" in sections:
    say(f"# tools/mb_mxfp6_rows.py on one {torch.cuda.get_device_name(0)} (gfx950): MXFP6 vs fp8 vs MXFP4 on the 3..8-row matrix-core GEMV (fragment-major weights).")
    say(f"# 1. rows GEMV at m = 8, us per launch as p50 (min - max) over {rounds} alternating rounds (dependent graph chain of 120 launches x 5 per round, "
        "device events) and TB/s of the bytes each form reads at the p50; `-`: the form does not cover the call (adaLN prologue beyond K = 2048)")
    L.check(lib.vv_tune(b"gemv_rows_scratch", 1), "scratch")
    for name, n, k, dual, kw in SHAPES:
        chains = {f: Chain(8, n, k, dual, f, **kw) for f in FORMS}
        live = [f for f in FORMS if chains[f].route is not None]
        t = {f: [] for f in live}
        for _ in range(rounds):
            for f in live:
                t[f].append(chains[f].time_us())
        mid = {f: p50(t[f]) for f in live}
        cols = "  ".join(f"{f} {mid[f]:6.2f} ({min(t[f]):6.2f} - {max(t[f]):6.2f}) us {chains[f].per / mid[f] / 1e6:5.2f} TB/s" if f in live else f"{f}      -"
                         for f in FORMS)
        ratio = f"mxfp6/fp8 time {mid['mxfp6'] / mid['fp8']:.2f}  mxfp6/mxfp4 time {mid['mxfp6'] / mid['mxfp4']:.2f}" if len(live) == 3 else ""
        say(f"{name:18s} n={n:5d} k={k:5d}{' dual' if dual else '     '}  {cols}   {ratio}   [{chains['mxfp6'].route}]")
        for c in chains.values():
            c.close()
        del chains
        torch.cuda.empty_cache()
    lib.vv_tune(b"gemv_rows_scratch", 0)

MODES = (("mxfp6 lanes", "mxfp6", {}, False), ("mxfp6 rows", "mxfp6", {"mxfp6_row_batch": True}, True), ("fp8 rows", "fp8", {}, True),
         ("mxfp4 rows", "mxfp4", {"mxfp4_row_batch": True}, True), ("bf16 rows", None, {}, True))

if "2" in sections:
    MODES = MODES[rotate % 5:] + MODES[:rotate % 5]
    say(f"# 2 (rotate={rotate}: built and timed in the order {', '.join(m[0] for m in MODES)}). generate() on B dialogues, {frames} forced speech frames each, injected noise, 20 steps; aggregate audio-sec/s as p50 (min - max) over {runs} runs "
        "per mode after a warm-up, the five modes alternating in one process.  `mxfp6 lanes` is the same commit with the keyword off (the default).")
    say("# The weights are synthetic: a waveform deviation says how far the arithmetic moves THIS random model's output, nothing about a checkpoint's audio quality.")
    for preset in presets:
        cfg = VVConfig.preset(preset)
        sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
        models = {}
        for name, wq, extra, _ in MODES:
            models[name] = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=wq, **extra)
            models[name].set_ddpm_inference_steps(20)
        del sd
        for B in batches:
            wls = [bench.build_workload(cfg, frames, 203, seed=201 + i) for i in range(B)]
            ids = torch.cat([w["input_ids"] for w in wls])
            kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=wls[0]["tok"], cfg_scale=2.0,
                      forced_tokens=[w["forced"] for w in wls], noise=torch.stack([w["noise"] for w in wls]),
                      speech_tensors=torch.cat([w["speech_tensors"] for w in wls]).cuda(),
                      speech_masks=torch.cat([w["speech_masks"] for w in wls]), speech_input_mask=torch.cat([w["speech_input_mask"] for w in wls]),
                      speech_noise=(torch.cat([w["speech_noise"][0] for w in wls]), torch.cat([w["speech_noise"][1] for w in wls])),
                      generation_config={"do_sample": False}, show_progress_bar=False,
                      max_length_times=max(2, -(-len(wls[0]["forced"]) // ids.shape[1]) + 1))
            rates, outs = {name: [] for name, *_ in MODES}, {}
            for i in range(runs + 2):                     # runs 0 and 1 warm every mode (lanes, graphs, the allocator's per-stream pools)
                for name, wq, extra, rows in MODES:
                    mdl = models[name]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = mdl.generate(**kw)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    assert bool(mdl._rowbatch) == rows, (name, list(mdl._rowbatch))
                    n = sum(o.shape[-1] for o in out.speech_outputs)
                    assert n == B * frames * cfg.hop, (n, B, frames)
                    outs[name] = np.concatenate([o.float().cpu().numpy().ravel() for o in out.speech_outputs])
                    if i > 1:
                        rates[name].append(n / 24000.0 / dt)
            for name, *_ in MODES:
                w = models[name].engine.w
                extra = f", of which MXFP6 fragment copies {w._frag_state['mxfp6_bytes'] / 1e9:.2f} GB = {w._frag_state['mxfp6_bytes'] / max(1, w._frag_state['mxfp6_weights']):.4f} B/weight" \
                    if w._frag_state["mxfp6_bytes"] else ""
                say(f"{preset} B={B} {name:11s}: {p50(rates[name]):7.2f} ({min(rates[name]):.2f} - {max(rates[name]):.2f}) audio-sec/s, device weights {w.nbytes() / 1e9:.2f} GB{extra}")
            a, r = outs["mxfp6 rows"], outs["mxfp6 lanes"]
            e = float(np.sqrt(np.mean((a - r) ** 2)) / max(np.sqrt(np.mean(r ** 2)), 1e-30))
            ok = bool(np.isfinite(a).all()) and e < 1.0
            say(f"{preset} B={B} mxfp6 rows vs mxfp6 lanes waveform: rel RMS {e:.3e} {'(finite)' if ok else '(WRONG OUTPUT: speed figure void)'}")
            gain = min(rates["mxfp6 rows"]) > max(rates["mxfp6 lanes"])
            say(f"{preset} B={B} mxfp6 rows / mxfp6 lanes {p50(rates['mxfp6 rows']) / p50(rates['mxfp6 lanes']):.3f} ({'rows min > lanes max' if gain else 'NO GAIN: rows min <= lanes max'})   "
                f"mxfp6 rows / fp8 rows {p50(rates['mxfp6 rows']) / p50(rates['fp8 rows']):.3f}   mxfp6 rows / mxfp4 rows {p50(rates['mxfp6 rows']) / p50(rates['mxfp4 rows']):.3f}   "
                f"mxfp6 rows / bf16 rows {p50(rates['mxfp6 rows']) / p50(rates['bf16 rows']):.3f}")
            for mdl in models.values():
                mdl.release_lanes()
        del models, mdl
        gc.collect()                                      # the engines hand their HIP streams back before the next preset builds its own
        torch.cuda.empty_cache()

if "3" in sections:
    section_3()
