"""Row-batched conv tails (batched_conv_rows, csrc/vv_conv_hot.hip) against the per-dialogue tails, one process, alternating legs, p50 (min - max):
  composites  on the real 1.5B nets, in a dependent hipGraph chain of 20 frames: vv_decoder_front_rows and vv_encoder_back_rows at B = 2, 4, 8
              against B times the same part of the per-dialogue composites (vv_decoder_forward minus vv_decoder_forward_from, vv_encoder_forward
              minus vv_encoder_forward_until); the routes of the vv_linear calls the new composites make (vv_linear_route)
  generate    bench.batched_leg (225 frames, forced schedule, 1.5B bf16) with the flag off against on: aggregate audio-sec/s at 4, 8 and 16
              dialogues, row_batch_width 4 and 8; with VV_RB_TIMING=1 in the environment the row batches print their per-step A / H / tails /
              step period (the back runs in front of A: it shows in the period and the gap, not in "tails")
  session     one 8-slot session with 16 dialogues of 60..225 frames submitted up front, flag off against on
    python tools/mb_conv_rows.py [composites] [generate[=4,8,16]] [session] [reps=2] > profiles/conv_rows.txt"""
import ctypes as C
import random
import statistics
import sys
import time
import types

ROOT = __file__.rsplit("/tools/", 1)[0]
sys.path.insert(0, ROOT)
sys.path.insert(0, ROOT + "/tools")
import torch

what = [a for a in sys.argv[1:] if not a.startswith("reps=")] or ["composites", "generate", "session"]
reps = next((int(a[5:]) for a in sys.argv[1:] if a.startswith("reps=")), 2)


def p50(v):
    return f"{statistics.median(v):7.2f} ({min(v):.2f} - {max(v):.2f})"


from vibevoice_rocm_amd import _lib as L
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
from vibevoice_rocm_amd.synth import synth_state_dict_torch

cfg = VVConfig.preset("1.5b")
sd = synth_state_dict_torch(cfg, 2024, device="cuda:0", dtype=torch.bfloat16)
m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
m.set_ddpm_inference_steps(20)
lib = m.engine.lib

if "composites" in what:
    CH = 20
    st = torch.cuda.Stream()
    sp = st.cuda_stream
    root = m.engine.w
    f32 = dict(dtype=torch.float32, device="cuda:0")
    u8 = dict(dtype=torch.uint8, device="cuda:0")

    def chain_us(fn):
        """us per call of fn() in a captured chain of CH dependent calls (same stream, same state: every call waits for the one before)"""
        st.synchronize()
        L.check(lib.vv_graph_begin(sp), "begin")
        for _ in range(CH):
            fn()
        ge = C.c_void_p()
        L.check(lib.vv_graph_end(sp, C.byref(ge)), "end")
        ts = []
        for i in range(8):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                e0.record(st)
                L.check(lib.vv_graph_launch(ge, sp), "launch")
                e1.record(st)
            st.synchronize()
            if i >= 2:
                ts.append(e0.elapsed_time(e1) * 1e3 / CH)
        lib.vv_graph_destroy(ge)
        return statistics.median(ts)

    dec_ws = torch.empty(lib.vv_convnet_ws_bytes(C.byref(root.dec), 1, 1), **u8)
    sem_ws = torch.empty(lib.vv_convnet_ws_bytes(C.byref(root.sem), cfg.hop, 0), **u8)
    print(f"per composite, 1.5B tokenizers (8 one-row blocks per net), us per call in a chain of {CH}: p50 (min - max) of 5 alternating rounds")
    for B in (2, 4, 8):
        ws = [root.fork() for _ in range(B)]
        dec = (C.POINTER(L.ConvNet) * B)(*[C.pointer(w.dec) for w in ws])
        sem = (C.POINTER(L.ConvNet) * B)(*[C.pointer(w.sem) for w in ws])
        act = torch.ones(B, dtype=torch.int32, device="cuda:0")
        lat = torch.randn(B, cfg.latent, **f32)
        mid, mid2 = torch.zeros(B, 8192, **f32), torch.randn(B, 8192, **f32)
        wav, feat = torch.randn(B, cfg.hop, **f32) * 0.1, torch.zeros(B, cfg.sem_dim, **f32)
        fws = torch.empty(lib.vv_conv_rows_ws_bytes(C.byref(root.dec), B, 1), **u8)
        bws = torch.empty(lib.vv_conv_rows_ws_bytes(C.byref(root.sem), B, 0), **u8)
        w0 = ws[0]
        legs = dict(
            front=lambda: L.check(lib.vv_decoder_front_rows(dec, B, act.data_ptr(), lat.data_ptr(), cfg.latent, 1.0, 0.0, mid.data_ptr(), 8192, fws.data_ptr(), sp), "front"),
            back=lambda: L.check(lib.vv_encoder_back_rows(sem, B, act.data_ptr(), mid2.data_ptr(), 8192, feat.data_ptr(), cfg.sem_dim, bws.data_ptr(), sp), "back"),
            dec_full=lambda: L.check(lib.vv_decoder_forward(C.byref(w0.dec), lat.data_ptr(), 1, 1.0, 0.0, wav.data_ptr(), dec_ws.data_ptr(), sp), "dec"),
            dec_from=lambda: L.check(lib.vv_decoder_forward_from(C.byref(w0.dec), mid.data_ptr(), wav.data_ptr(), dec_ws.data_ptr(), sp), "from"),
            sem_full=lambda: L.check(lib.vv_encoder_forward(C.byref(w0.sem), wav.data_ptr(), cfg.hop, feat.data_ptr(), sem_ws.data_ptr(), sp), "sem"),
            sem_until=lambda: L.check(lib.vv_encoder_forward_until(C.byref(w0.sem), wav.data_ptr(), cfg.hop, mid2.data_ptr(), sem_ws.data_ptr(), sp), "until"))
        t = {k: [] for k in legs}
        for _ in range(5):
            for k, fn in legs.items():
                t[k].append(chain_us(fn))
        d1 = [a - b for a, b in zip(t["dec_full"], t["dec_from"])]
        s1 = [a - b for a, b in zip(t["sem_full"], t["sem_until"])]
        print(f"  B = {B}: vv_decoder_front_rows {p50(t['front'])} us   per dialogue: one-row part of vv_decoder_forward {p50(d1)} us (full {p50(t['dec_full'])}, "
              f"from {p50(t['dec_from'])}) -> x {B} = {B * statistics.median(d1):.1f} us", flush=True)
        print(f"         vv_encoder_back_rows  {p50(t['back'])} us   per dialogue: one-row part of vv_encoder_forward {p50(s1)} us (full {p50(t['sem_full'])}, "
              f"until {p50(t['sem_until'])}) -> x {B} = {B * statistics.median(s1):.1f} us", flush=True)
        del ws
    print("routes of the vv_linear calls inside the new composites (the 18 big matrices run on rows_gemv_kernel / row_in_rows_kernel, csrc/vv_conv_hot.hip):")
    buf = C.create_string_buffer(128)
    dummy = torch.zeros(8, 16384, **f32)
    for name, mm, n, k, ldx in (("decoder stem conv, per dialogue", 1, 2048, 7 * cfg.ac_dim, cfg.ac_dim), ("encoder head conv, B rows", 8, cfg.sem_dim, 7 * 2048, 9 * 2048),
                                ("encoder head conv, B rows", 4, cfg.sem_dim, 7 * 2048, 9 * 2048), ("connector fc2, B rows", 8, cfg.hidden, cfg.hidden, cfg.hidden),
                                ("connector fc2, B rows", 4, cfg.hidden, cfg.hidden, cfg.hidden)):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.ldo = dummy.data_ptr(), ldx, mm, n, k, L.VV_BF16, n
        a.w, a.out, a.bias = root.embed.data_ptr(), dummy.data_ptr(), dummy.data_ptr()
        rc = lib.vv_linear_route(C.byref(a), buf, 128)
        print(f"  {name:<34} m={mm} n={n:5d} k={k:5d}: {buf.value.decode() if rc == 0 else 'rc=%d' % rc}")

gen = next((a for a in what if a.startswith("generate")), None)
if gen or "session" in what:
    import bench

if gen:
    args = types.SimpleNamespace(frames=225, voice_frames=203, cfg_scale=2.0)
    batches = [int(v) for v in gen.split("=")[1].split(",")] if "=" in gen else [4, 8, 16]
    print(f"generate(): aggregate audio-sec/s, p50 (min - max) of {3 * reps} timed calls per leg (legs alternate; two warm-up calls in front of each three)")
    for B in batches:
        for w in ((4,) if B <= 4 else (4, 8)):
            runs = {False: [], True: []}
            m.row_batch_width = w
            for _ in range(reps):
                for on in (False, True):
                    m.batched_conv_rows = on
                    runs[on] += bench.batched_leg(m, cfg, args, B, row_batch=True)["runs"]
            m.batched_conv_rows = False
            print(f"  {B:2d} dialogues, width {w}: flag off {p50(runs[False])}   flag on {p50(runs[True])}   "
                  f"ratio {statistics.median(runs[True]) / statistics.median(runs[False]):.3f}", flush=True)
    m.row_batch_width = 4

if "session" in what:
    N, slots = 16, 8
    frames = [60 + round(i * 165 / (N - 1)) for i in range(N)]
    random.Random(7).shuffle(frames)
    wls = [bench.build_workload(cfg, frames[i], 203, seed=301 + i) for i in range(N)]
    tok, L0 = wls[0]["tok"], wls[0]["input_ids"].shape[1]
    runs = {False: [], True: []}
    for r in range(reps + 1):              # the first round warms up (graphs, lanes) and is dropped
        for on in (False, True):
            m.batched_conv_rows = on
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
                runs[on].append(n / 24000.0 / (time.perf_counter() - t0))
    m.batched_conv_rows = False
    print(f"session, {slots} slots, {N} dialogues of 60..225 frames: flag off {p50(runs[False])}   flag on {p50(runs[True])} audio-sec/s", flush=True)
