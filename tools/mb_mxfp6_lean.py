"""mxfp6_lean, measured: the GEMM on MXFP6 codes against the route the bf16 copy of the same matrix takes (what an mxfp6 model with copies runs)
and against the GEMM on MXFP4 codes on the same shapes, one prefill pass and the first-chunk latency of a lean model against the same model
with its bf16 copies, and the bytes both hold.  Synthetic weights, weight_quant="mxfp6".

  gemm         the 1.5B and 7B prefill matrices (qkv, o, gate + up as the dual SwiGLU GEMM with a bf16 output, down) at M = 89, 330, 1 320 and
               2 640 rows: vv_linear on the VV_MXFP6 companion with VV_LIN_W_MX6GEMM, on the bf16 matrix of the same effective weights (the call
               llm_forward's prefill branch makes for a model that has the copy) and on a VV_MXFP4 companion of the same shape with
               VV_LIN_W_MXGEMM, alternating in one process.  p50 (min - max) of the repetitions in us, TFLOP/s from the shapes (2 m n k, twice
               that for the dual GEMM).  A cell where the GEMM on the MXFP6 codes is slower than the reference beside it is printed in **bold**.
  pass         Engine.prefill of 89, 330, 1 320 and 2 640 rows (+ the negative row) as one pass on both 1.5B models, alternating; host clock
               around work that ends in a stream synchronise.
  first_chunk  generate() entry to the first audio chunk on the host, one headline dialogue (4 voices, 203 text tokens), both 1.5B models.
  memory       DeviceWeights.nbytes() and torch.cuda.memory_allocated() after construction: copies / lean / lean + mxfp6_row_batch (fragment
               copies built), 1.5B and 7B, bytes per quantised weight.
--lib PATH loads another build of the library (a tile variant of csrc/vv_gemm_mx6.hip: hipcc -DVV_MX6_CG=1 | 2 | 4, 32 / 64 / 128 channels per
workgroup tile); the gemm leg then says which.
Every timed leg warms its shapes first and alternates its versions.    python tools/mb_mxfp6_lean.py [leg ...] [--reps N] [--lib PATH]"""
import ctypes as C
import gc
import sys
import time
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
import bench
from vibevoice_rocm_amd import _lib as L

argv = sys.argv[1:]
if "--lib" in argv:
    L.LIB_PATH = argv[argv.index("--lib") + 1]
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch
from vibevoice_rocm_amd.weights import fp8_matrix_names, pack_mxfp4, pack_mxfp6, quantize_mxfp4, quantize_mxfp6

opt = {k: int(argv[argv.index(k) + 1]) for k in ("--reps",) if k in argv}
ALL = ("gemm", "pass", "first_chunk", "memory")
legs = [a for a in argv if a in ALL] or list(ALL)
REPS = opt.get("--reps", 5)
ROWS = (89, 330, 1320, 2640)
lib = L.load()
L.check(lib.vv_init(), "vv_init")
fmt = lambda v, d=1: f"{sorted(v)[len(v) // 2]:.{d}f} ({min(v):.{d}f} - {max(v):.{d}f})"      # noqa: E731
p50 = lambda v: sorted(v)[len(v) // 2]      # noqa: E731
bold = lambda s, on: f"**{s}**" if on else s      # noqa: E731


def leg_gemm():
    shapes = []
    for name in ("1.5b", "7b"):
        c = VVConfig.preset(name)
        qd, qkvd = c.heads * c.head_dim, (c.heads + 2 * c.kv_heads) * c.head_dim
        shapes += [(name, "qkv", qkvd, c.hidden, 0), (name, "o", c.hidden, qd, 0), (name, "gate+up", c.inter, c.hidden, 1), (name, "down", c.hidden, c.inter, 0)]
    print(f"library: {L.LIB_PATH}")
    print(f"{'model':<5} {'matrix':<8} {'n':>6} {'k':>6} {'m':>5}  {'route of the bf16 copy':<38} {'bf16 us p50 (min - max)':>28} {'TF/s':>6}  "
          f"{'gemm_mx us p50 (min - max)':>28} {'TF/s':>6}  {'gemm_mx6 us p50 (min - max)':>30} {'TF/s':>6}  {'bf16 / mx6':>10} {'mx / mx6':>9}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for model, mat, n, k, dual in shapes:
        ws = []
        for _ in range(1 + dual):
            w = (torch.randn(n, k, device="cuda", generator=g) / k ** 0.5).bfloat16()
            c6, s6, eff = quantize_mxfp6(w)
            c4, s4, _ = quantize_mxfp4(w)
            ws.append((eff.bfloat16().contiguous(), pack_mxfp4(c4, s4), pack_mxfp6(c6, s6)))
        for m in ROWS:
            x = torch.randn(m, k, device="cuda", generator=g).bfloat16()
            out = torch.empty(m, n, device="cuda", dtype=torch.bfloat16 if dual else torch.float32)
            args = []
            for v in (0, 1, 2):      # 0: the bf16 copy, 1: gemm_mx on MXFP4 codes, 2: gemm_mx6 on MXFP6 codes
                a = L.LinArgs()
                a.x, a.ldx, a.m, a.n, a.k, a.out, a.ldo = x.data_ptr(), k, m, n, k, out.data_ptr(), n
                a.flags = L.LIN_X_BF16 | (L.LIN_OUT_BF16 if dual else 0) | (0, L.LIN_W_MXGEMM, L.LIN_W_MX6GEMM)[v]
                a.wdt = (L.VV_BF16, L.VV_MXFP4, L.VV_MXFP6)[v]
                a.w = ws[0][0].data_ptr() if v == 0 else ws[0][v][0].data_ptr()
                if v:
                    a.wscale = ws[0][v][1].data_ptr()
                if dual:
                    a.act, a.w2 = L.ACT_SWIGLU, (ws[1][0] if v == 0 else ws[1][v][0]).data_ptr()
                    if v:
                        a.w2scale = ws[1][v][1].data_ptr()
                args.append(a)
            name = C.create_string_buffer(96)
            L.check(lib.vv_linear_route(C.byref(args[0]), name, 96), "route")
            parent = name.value.decode()
            L.check(lib.vv_linear_route(C.byref(args[2]), name, 96), "route")
            assert name.value.decode().startswith("gemm_mx6"), name.value
            flops = 2.0 * m * n * k * (2 if dual else 1)
            inner = max(3, min(50, int(2e-3 * 3e14 / flops)))       # ~ 2 ms of work per timed window at 300 TF/s
            t = {0: [], 1: [], 2: []}
            for rep in range(REPS + 2):                              # two warm-up rounds of every version
                for v in (0, 1, 2):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(inner):
                        L.check(lib.vv_linear(C.byref(args[v]), None), "vv_linear")
                    e1.record()
                    e1.synchronize()
                    if rep >= 2:
                        t[v].append(e0.elapsed_time(e1) * 1e3 / inner)
            tf = lambda us: flops / (us * 1e-6) / 1e12      # noqa: E731
            a0, a1, a2 = p50(t[0]), p50(t[1]), p50(t[2])
            print(f"{model:<5} {mat:<8} {n:>6} {k:>6} {m:>5}  {parent:<38} {fmt(t[0]):>28} {tf(a0):>6.0f}  {fmt(t[1]):>28} {tf(a1):>6.0f}  {fmt(t[2]):>30} {tf(a2):>6.0f}  "
                  f"{bold(f'{a0 / a2:.2f}', a2 > a0):>10} {bold(f'{a1 / a2:.2f}', a2 > a1):>9}", flush=True)


def build(preset, **kw):
    cfg = VVConfig.preset(preset)
    sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", **kw)
    m.set_ddpm_inference_steps(20)
    return cfg, m


def leg_pass(cfg, models):
    V = cfg.vocab
    g = torch.Generator().manual_seed(3)
    for name, m in models.items():
        m.engine.begin_sequence(4096, [V - 4, V - 3, V - 2, V - 1])
    for rows in ROWS:
        emb = (0.5 * torch.randn(rows, cfg.hidden, generator=g)).cuda()
        t = {name: [] for name in models}
        for rep in range(REPS + 2):
            for name, m in models.items():
                eng = m.engine
                neg = eng.embed_ids(torch.tensor([V - 4]))
                eng.stream.synchronize()
                t0 = time.perf_counter()
                eng.prefill(emb, neg_embed=neg, chunk=4096)
                eng.stream.synchronize()
                if rep >= 2:
                    t[name].append((time.perf_counter() - t0) * 1e3)
        r = p50(t['copies']) / p50(t['lean'])
        print(f"prefill pass, 1.5B, {rows} rows + the negative row: bf16 copies {fmt(t['copies'], 2)} ms, lean {bold(fmt(t['lean'], 2), r < 1)} ms, "
              f"copies / lean {bold(f'{r:.2f}', r < 1)}", flush=True)


def leg_first_chunk(cfg, models):
    from vibevoice_rocm_amd.streamer import AudioStreamer

    class Timer(AudioStreamer):
        def __init__(self):
            super().__init__(batch_size=1)
            self.first = None

        def put(self, audio_chunks, sample_indices):
            audio_chunks[0].detach().cpu()
            if self.first is None:
                self.first = time.perf_counter()

    w = bench.build_workload(cfg, 4, 203, seed=401)
    SD = w["special"]["speech_diffusion"]
    t = {name: [] for name in models}
    for rep in range(REPS + 2):
        for name, m in models.items():
            st = Timer()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(input_ids=w["input_ids"], tokenizer=w["tok"], cfg_scale=2.0, forced_tokens=[SD] * 2 + w["forced"][-2:], noise=w["noise"],
                       speech_tensors=w["speech_tensors"].to(m.device), speech_masks=w["speech_masks"], speech_input_mask=w["speech_input_mask"],
                       speech_noise=w["speech_noise"], generation_config={"do_sample": False}, audio_streamer=st)
            if rep >= 2:
                t[name].append((st.first - t0) * 1e3)
    r = p50(t['copies']) / p50(t['lean'])
    print(f"first chunk (voice encode + prefill + first frame, prompt of {w['input_ids'].shape[1]} tokens), 1.5B: bf16 copies {fmt(t['copies'], 2)} ms, "
          f"lean {bold(fmt(t['lean'], 2), r < 1)} ms, copies / lean {bold(f'{r:.2f}', r < 1)}", flush=True)


def leg_memory():
    for preset in ("1.5b", "7b"):
        cfg = VVConfig.preset(preset)
        seen = {}
        sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
        nq = sum(sd[k].numel() for k in fp8_matrix_names(cfg))
        del sd
        for what, kw in (("copies", {}), ("lean", dict(mxfp6_lean=True)), ("lean + row batch", dict(mxfp6_lean=True, mxfp6_row_batch=True))):
            gc.collect()
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            _, m = build(preset, **kw)
            if kw.get("mxfp6_row_batch"):
                m.engine.w.ensure_frag()
            torch.cuda.synchronize()
            gc.collect()
            nb, alloc = m.engine.w.nbytes(), torch.cuda.memory_allocated() - base
            dropped = sum(d["bytes"] for d in m.engine.w.lean_report())
            seen[what] = nb
            print(f"{preset} mxfp6 {what}: nbytes {nb / 1e9:.3f} GB, memory_allocated {alloc / 1e9:.3f} GB, "
                  f"dropped bf16 copies {dropped / 1e9:.3f} GB ({len(m.engine.w.lean_report())} matrices), {nq / 1e9:.3f} G quantised weights", flush=True)
            del m
        d = seen["copies"] - seen["lean"]
        print(f"{preset}: lean saves {d / 1e9:.3f} GB = {d / nq:.3f} B per quantised weight", flush=True)


print(f"{torch.cuda.get_device_name(0)}; {REPS} alternating repetitions per figure after two warm-up rounds", flush=True)
if "gemm" in legs:
    leg_gemm()
if "pass" in legs or "first_chunk" in legs:
    cfg, copies = build("1.5b")
    _, lean = build("1.5b", mxfp6_lean=True)
    models = {"copies": copies, "lean": lean}
    if "pass" in legs:
        leg_pass(cfg, models)
    if "first_chunk" in legs:
        leg_first_chunk(cfg, models)
    del models, copies, lean
if "memory" in legs:
    leg_memory()
