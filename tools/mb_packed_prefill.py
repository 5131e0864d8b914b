"""Packed prompt prefill, measured: the LDS-DMA tile GEMM against today's route per matrix, one prefill pass packed against per dialogue, the
first-chunk latency of batched generate() and a serving session with packed admission on against off.  bf16, synthetic weights.

  gemm         the 1.5B and 7B prefill matrices (qkv, o, gate + up as the dual SwiGLU GEMM with a bf16 output, down) at M = 128 .. 4096 rows:
               vv_linear with VV_LIN_PACKED under vv_tune("gemm_packed_rows", 1) against the same arguments without the flag, alternating in
               one process.  p50 (min - max) of the repetitions in us, TFLOP/s from the shapes (2 m n k, twice that for the dual GEMM) and the
               share of the 2.5 PFLOP/s dense bf16 matrix-core peak (all of these GEMMs are compute bound at these row counts).
  pass         RowBatch.prefill_packed against RowBatch.prefill per dialogue, 1.5B: B = 2, 4, 8 dialogues of 330 prompt rows, and of 89 rows
               behind a 241-slot voice prefix; host clock around work that ends in a stream synchronise.
  first_chunk  generate() entry to the first chunk of every dialogue on the host, 4 and 8 headline dialogues, packed_prefill on against off.
  session      tools/mb_session.py's workload through one 8-slot session, packed admission on against off: audio-sec/s, mean stall per admission wave.
Every leg warms its shapes first and alternates its versions.    python tools/mb_packed_prefill.py [leg ...] [--reps N] [--rows R]"""
import ctypes as C
import random
import sys
import time
sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
import torch
import bench
from vibevoice_rocm_amd import _lib as L
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch

argv = sys.argv[1:]
opt = {k: int(argv[argv.index(k) + 1]) for k in ("--reps", "--rows") if k in argv}
legs = [a for a in argv if a in ("gemm", "pass", "first_chunk", "session")] or ["gemm", "pass", "first_chunk", "session"]
REPS = opt.get("--reps", 15)
PEAK = 2.5e15
lib = L.load()
L.check(lib.vv_init(), "vv_init")
if "--rows" in opt:
    L.check(lib.vv_tune(b"gemm_packed_rows", opt["--rows"]), "vv_tune")
fmt = lambda v, d=1: f"{sorted(v)[len(v) // 2]:.{d}f} ({min(v):.{d}f} - {max(v):.{d}f})"      # noqa: E731
p50 = lambda v: sorted(v)[len(v) // 2]      # noqa: E731


def leg_gemm():
    shapes = []
    for name in ("1.5b", "7b"):
        c = VVConfig.preset(name)
        qd, qkvd = c.heads * c.head_dim, (c.heads + 2 * c.kv_heads) * c.head_dim
        shapes += [(name, "qkv", qkvd, c.hidden, 0), (name, "o", c.hidden, qd, 0), (name, "gate+up", c.inter, c.hidden, 1), (name, "down", c.hidden, c.inter, 0)]
    print(f"{'model':<5} {'matrix':<8} {'n':>6} {'k':>6} {'m':>5}  {'parent route':<34} {'parent us p50 (min - max)':>28} {'TF/s':>6} {'peak':>6}  "
          f"{'gemm_packed us p50 (min - max)':>30} {'TF/s':>6} {'peak':>6}  {'speed-up':>8}", flush=True)
    g = torch.Generator(device="cuda").manual_seed(1)
    for model, mat, n, k, dual in shapes:
        w = (torch.randn(n, k, device="cuda", generator=g) / k ** 0.5).bfloat16()
        w2 = (torch.randn(n, k, device="cuda", generator=g) / k ** 0.5).bfloat16() if dual else None
        for m in (128, 330, 712, 1320, 2640, 4096):
            x = torch.randn(m, k, device="cuda", generator=g).bfloat16()
            out = torch.empty(m, n, device="cuda", dtype=torch.bfloat16 if dual else torch.float32)
            a = L.LinArgs()
            a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo = x.data_ptr(), k, m, n, k, L.VV_BF16, w.data_ptr(), out.data_ptr(), n
            a.flags = L.LIN_X_BF16 | (L.LIN_OUT_BF16 if dual else 0)
            if dual:
                a.w2, a.act = w2.data_ptr(), L.ACT_SWIGLU
            name = C.create_string_buffer(96)
            L.check(lib.vv_linear_route(C.byref(a), name, 96), "route")
            parent = name.value.decode()
            flops = 2.0 * m * n * k * (2 if dual else 1)
            inner = max(3, min(50, int(2e-3 * 3e14 / flops)))       # ~ 2 ms of work per timed window at 300 TF/s
            t = {0: [], 1: []}
            for rep in range(REPS + 2):                              # two warm-up rounds of both versions
                for packed in (0, 1):
                    a.flags = (a.flags & ~L.LIN_PACKED) | (L.LIN_PACKED if packed else 0)
                    L.check(lib.vv_tune(b"gemm_packed_rows", 1 if packed else 0), "vv_tune")
                    if packed and rep == 0:
                        L.check(lib.vv_linear_route(C.byref(a), name, 96), "route")
                        assert name.value.decode().startswith("gemm_packed"), name.value
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(inner):
                        L.check(lib.vv_linear(C.byref(a), None), "vv_linear")
                    e1.record()
                    e1.synchronize()
                    if rep >= 2:
                        t[packed].append(e0.elapsed_time(e1) * 1e3 / inner)
            tf = lambda us: flops / (us * 1e-6) / 1e12      # noqa: E731
            a0, a1 = p50(t[0]), p50(t[1])
            print(f"{model:<5} {mat:<8} {n:>6} {k:>6} {m:>5}  {parent:<34} {fmt(t[0]):>28} {tf(a0):>6.0f} {tf(a0) * 1e12 / PEAK:>6.1%}  "
                  f"{fmt(t[1]):>30} {tf(a1):>6.0f} {tf(a1) * 1e12 / PEAK:>6.1%}  {a0 / a1:>8.2f}", flush=True)
    L.check(lib.vv_tune(b"gemm_packed_rows", opt.get("--rows", -1)), "vv_tune")


def model_15b():
    cfg = VVConfig.preset("1.5b")
    sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m.set_ddpm_inference_steps(20)
    return cfg, m


def leg_pass(cfg, m):
    from vibevoice_rocm_amd.rowbatch import RowBatch
    V, eng = cfg.vocab, m.engine
    valid = [V - 4, V - 3, V - 2, V - 1]
    g = torch.Generator().manual_seed(3)
    eng.begin_sequence(512, valid)
    eng.prefill((0.5 * torch.randn(241, cfg.hidden, generator=g)).cuda())
    vp = eng.save_prefix(torch.arange(241))
    neg = eng.embed_ids(torch.tensor([V - 4]))
    for B in (2, 4, 8):
        rb = RowBatch([m._lane(b) for b in range(B)], stream=eng.stream)
        rb.begin(512, valid, 1.0)
        for rows, prefix in ((330, None), (89, vp)):
            emb = [(0.5 * torch.randn(rows, cfg.hidden, generator=g)).cuda() for _ in range(B)]
            items = [(b, emb[b], prefix) for b in range(B)]

            def per_dialogue():
                for b, e, p in items:
                    rb.prefill(b, e, neg_embed=neg, prefix=p)

            def packed():
                rb.prefill_packed(items, chunk_rows=m.packed_prefill_rows, neg_embed=neg)
            t = {"per dialogue": [], "packed": []}
            for rep in range(REPS + 2):
                for name, fn in (("per dialogue", per_dialogue), ("packed", packed)):
                    rb.stream.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    rb.stream.synchronize()
                    if rep >= 2:
                        t[name].append((time.perf_counter() - t0) * 1e3)
            print(f"prefill pass, 1.5B, B = {B} x {rows} rows{' behind a 241-slot prefix' if prefix else ''}: per dialogue {fmt(t['per dialogue'], 2)} ms, "
                  f"packed {fmt(t['packed'], 2)} ms, ratio {p50(t['per dialogue']) / p50(t['packed']):.2f}", flush=True)
        rb.close()


def leg_first_chunk(cfg, m):
    from vibevoice_rocm_amd.streamer import AudioStreamer

    class Timer(AudioStreamer):
        def __init__(self, B):
            super().__init__(batch_size=B)
            self.first = {}

        def put(self, audio_chunks, sample_indices):
            audio_chunks[0].detach().cpu()
            for i in sample_indices:
                self.first.setdefault(int(i), time.perf_counter())

    for B in (4, 8):
        wls = [bench.build_workload(cfg, 4, 203, seed=401 + i) for i in range(B)]
        ids = torch.cat([w["input_ids"] for w in wls])
        SD = wls[0]["special"]["speech_diffusion"]
        kw = dict(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=wls[0]["tok"], cfg_scale=2.0, forced_tokens=[[SD] * 2 + w["forced"][-2:] for w in wls],
                  noise=torch.stack([w["noise"] for w in wls]), speech_tensors=torch.cat([w["speech_tensors"] for w in wls]).to(m.device),
                  speech_masks=torch.cat([w["speech_masks"] for w in wls]), speech_input_mask=torch.cat([w["speech_input_mask"] for w in wls]),
                  speech_noise=(torch.cat([w["speech_noise"][0] for w in wls]), torch.cat([w["speech_noise"][1] for w in wls])),
                  generation_config={"do_sample": False})
        t = {False: [], True: []}
        for rep in range(REPS + 2):
            for packed in (False, True):
                st = Timer(B)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m.generate(audio_streamer=st, packed_prefill=packed, **kw)
                if rep >= 2:
                    t[packed].append((max(st.first.values()) - t0) * 1e3)
        print(f"first chunk of all {B} dialogues (voice encode + prefill + first frame, prompts of {ids.shape[1]} tokens), 1.5B: packed_prefill off "
              f"{fmt(t[False], 2)} ms, on {fmt(t[True], 2)} ms, ratio {p50(t[False]) / p50(t[True]):.2f}", flush=True)


def leg_session(cfg, m, N=24, slots=8):
    frames = [60 + round(i * 165 / (N - 1)) for i in range(N)]
    random.Random(7).shuffle(frames)
    wls = [bench.build_workload(cfg, frames[i], 203, seed=301 + i) for i in range(N)]
    tok, L0 = wls[0]["tok"], wls[0]["input_ids"].shape[1]
    mlt = max(2, -(-(max(frames) + 2) // L0) + 1)
    res, stall = {False: [], True: []}, {False: [], True: []}
    for rep in range(min(REPS, 3) + 1):
        for packed in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with m.open_session(tokenizer=tok, slots=slots, max_context=L0 + max(frames) + 2 + 8 + 64, packed_prefill=packed) as sess:
                hs = [sess.submit(input_ids=w["input_ids"], cfg_scale=2.0, forced_tokens=w["forced"], speech_tensors=w["speech_tensors"].to(m.device),
                                  speech_masks=w["speech_masks"], speech_input_mask=w["speech_input_mask"], speech_noise=w["speech_noise"],
                                  max_length_times=mlt, max_new_tokens=len(w["forced"]), noise_seed=4000 + i) for i, w in enumerate(wls)]
                sess.run()
                ms = list(sess.admission_ms)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if rep:
                res[packed].append(sum(h.result().speech_outputs[0].shape[-1] for h in hs) / 24000.0 / dt)
                stall[packed].append((ms[0], sum(ms[1:]) / max(1, len(ms) - 1), len(ms)))
    for packed in (False, True):
        s = stall[packed]
        print(f"session, {N} dialogues on {slots} slots, 1.5B, packed admission {'on ' if packed else 'off'}: {fmt(res[packed], 2)} audio-sec/s; "
              f"{s[0][2]} admission waves, the first {p50([x[0] for x in s]):.1f} ms, mid-flight ones {p50([x[1] for x in s]):.2f} ms each (mean)", flush=True)


print(f"{torch.cuda.get_device_name(0)}; {REPS} alternating repetitions per figure after two warm-up rounds (session: at most 3 after one)", flush=True)
if "gemm" in legs:
    leg_gemm()
if set(legs) - {"gemm"}:
    cfg, model = model_15b()
    if "pass" in legs:
        leg_pass(cfg, model)
        model.release_lanes()
    if "first_chunk" in legs:
        leg_first_chunk(cfg, model)
        model.release_lanes()
    if "session" in legs:
        leg_session(cfg, model)
