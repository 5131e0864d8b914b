"""Weight-only fp8 on the row-batched decode path (rowbatch.py, the fp8 form of csrc/vv_gemv_rows.hip), 1.5B shapes, one process:

  1. per-launch us of the 8-row matrix-core GEMV on the frame's matrices, bf16 fragment-major vs fp8 fragment-major (a dependent hipGraph chain
     over enough weight copies that nothing is served from the caches; the residual projections in place, as the composites call them);
  2. generate() on 4 and 8 dialogues with the forced bench schedule (`frames` speech frames each): bf16 row-batched, fp8 on the lanes and fp8
     row-batched, alternating in one process after a warm-up call of each.  Prints audio-sec/s per call and the medians.
    python tools/mb_rowbatch_fp8.py [frames=225] [batches=4,8] [timed calls per leg=3]"""
import ctypes as C
import sys
import time
import types

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
import bench
from vibevoice_rocm_amd import _lib as L
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch
from vibevoice_rocm_amd.weights import DeviceWeights, quantize_e4m3_pow2

frames = int(sys.argv[1]) if len(sys.argv) > 1 else 225
batches = [int(v) for v in (sys.argv[2].split(",") if len(sys.argv) > 2 else ("4", "8"))]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
lib = L.load()
L.check(lib.vv_init(), "vv_init")

# ---- 1. per-launch GEMV time -------------------------------------------------------------------------------------------------------------------
SHAPES = (("head gate/up", 4608, 1536, True, dict(pro=1, mod=True, flags=L.LIN_W_REUSED)),
          ("head down", 1536, 4608, False, dict(epi=True, flags=L.LIN_W_REUSED)),
          ("llm qkv", 2048, 1536, False, dict(pro=1, bias=True)), ("llm o", 1536, 1536, False, dict(epi=True)),
          ("llm gate/up", 8960, 1536, True, dict(pro=1)), ("llm down", 1536, 8960, False, dict(epi=True)))


def chain_us(m, n, k, dual, fp8, pro=0, mod=False, epi=False, bias=False, flags=0, N=120):
    """mean us per launch of N dependent vv_linear launches in one graph; weights cycle through enough copies to exceed 1 GB"""
    st = torch.cuda.Stream()
    copies = max(2, int(1.2e9 // (n * k * (1 if fp8 else 2) * (2 if dual else 1))))
    copies = min(copies, N)
    with torch.cuda.stream(st):
        ld = max(n, k)
        bufs = [torch.randn(m, ld, device="cuda") * 0.5 for _ in range(2)]
        ws = []
        for _ in range(copies):
            mats = []
            for _j in range(2 if dual else 1):
                w = torch.randn(n, k, device="cuda") / k ** 0.5
                if fp8:
                    q, s, _ = quantize_e4m3_pow2(w)
                    mats.append((DeviceWeights.frag_major_fp8(q), s))
                else:
                    mats.append((DeviceWeights.frag_major(w.bfloat16()), None))
            ws.append(mats)
        nw = torch.ones(k, device="cuda")
        sh, sc = torch.zeros(m, k, device="cuda"), torch.zeros(m, k, device="cuda")
        gate, b = torch.full((m, n), 0.5, device="cuda"), torch.zeros(n, device="cuda")
        args = []
        for i in range(N):
            a = L.LinArgs()
            a.x, a.ldx, a.m, a.n, a.k = bufs[i & 1].data_ptr(), ld, m, n, k
            a.out, a.ldo = bufs[(i + 1) & 1].data_ptr(), ld
            a.pro, a.norm_w, a.eps = pro, (nw.data_ptr() if pro == 1 else 0), 1e-5
            a.flags = flags | L.LIN_W_FRAG
            if mod:
                a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
            mats = ws[i % copies]
            a.wdt = L.VV_FP8 if fp8 else L.VV_BF16
            a.w = mats[0][0].data_ptr()
            if fp8:
                a.wscale = mats[0][1].data_ptr()
            if dual:
                a.w2, a.act = mats[1][0].data_ptr(), 2
                if fp8:
                    a.w2scale = mats[1][1].data_ptr()
            if epi:             # residual in place, as the composites call it (long K: the atomic split-K form)
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
            t0 = time.perf_counter()
            for _ in range(5):
                lib.vv_graph_launch(ge, st.cuda_stream)
            st.synchronize()
            best = min(best, (time.perf_counter() - t0) / 5 / N * 1e6)
        lib.vv_graph_destroy(ge)
    del ws
    torch.cuda.empty_cache()
    return best, n * k * (1 if fp8 else 2) * (2 if dual else 1)


L.check(lib.vv_tune(b"gemv_rows_scratch", 1), "scratch")
for name, n, k, dual, kw in SHAPES:
    t16, b16 = chain_us(8, n, k, dual, False, **kw)
    t8, b8 = chain_us(8, n, k, dual, True, **kw)
    print(f"{name:13s} n={n:5d} k={k:5d} 8 rows: bf16 frag {t16:6.2f} us ({b16 / t16 / 1e6:.2f} TB/s)   fp8 frag {t8:6.2f} us "
          f"({b8 / t8 / 1e6:.2f} TB/s)   fp8 / bf16 {t8 / t16:.2f}", flush=True)
L.check(lib.vv_tune(b"gemv_rows_scratch", 0), "scratch")

# ---- 2. generate() -----------------------------------------------------------------------------------------------------------------------------
cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
models = {q: VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=q) for q in (None, "fp8")}
for mm in models.values():
    mm.set_ddpm_inference_steps(20)
LEGS = (("bf16 row-batched", None, True), ("fp8 lanes", "fp8", False), ("fp8 row-batched", "fp8", True))
args = types.SimpleNamespace(frames=frames, voice_frames=203, cfg_scale=2.0)
for batch in batches:
    wls = [bench.build_workload(cfg, frames, args.voice_frames, seed=201 + i) for i in range(batch)]
    ids = torch.cat([w["input_ids"] for w in wls])
    kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=wls[0]["tok"], cfg_scale=args.cfg_scale,
              forced_tokens=[w["forced"] for w in wls], speech_tensors=torch.cat([w["speech_tensors"] for w in wls]).cuda(),
              speech_masks=torch.cat([w["speech_masks"] for w in wls]), speech_input_mask=torch.cat([w["speech_input_mask"] for w in wls]),
              speech_noise=(torch.cat([w["speech_noise"][0] for w in wls]), torch.cat([w["speech_noise"][1] for w in wls])),
              noise=torch.stack([w["noise"] for w in wls]),
              show_progress_bar=False, max_length_times=max(2, -(-len(wls[0]["forced"]) // ids.shape[1]) + 1))
    rates = {leg[0]: [] for leg in LEGS}
    for mm in models.values():
        mm.release_lanes()
    for i in range(reps + 1):               # call 0 of each leg warms up (lanes, row batches, graph captures)
        for name, q, rb in LEGS:
            mm = models[q]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = mm.generate(row_batch=rb, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n = sum(o.shape[-1] for o in out.speech_outputs)
            assert n == batch * frames * cfg.hop, (n, batch, frames)
            assert not rb or mm._rowbatch, f"{name}: the row-batched path was not taken"
            if i:
                rates[name].append(n / 24000.0 / dt)
    med = {k: sorted(v)[len(v) // 2] for k, v in rates.items()}
    print(f"batch {batch}: " + ", ".join(f"{k} {med[k]:.1f} audio-sec/s (runs {', '.join(f'{v:.1f}' for v in rates[k])})" for k in rates)
          + f"; fp8 row-batched / bf16 row-batched {med['fp8 row-batched'] / med['bf16 row-batched']:.3f}, "
          f"/ fp8 lanes {med['fp8 row-batched'] / med['fp8 lanes']:.2f}", flush=True)
