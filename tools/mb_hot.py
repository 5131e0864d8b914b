"""Per-shape time of the six hot decode GEMVs on the generic template and on their own kernels (csrc/vv_gemv_hot.hip), through vv_linear
with the operands of the real call sites, inside a hipGraph chain of DEPENDENT launches (x of launch i is the output of launch i - 1;
the pattern of mb_chain_lin.py / mb_nopro.py).  Weights cycle through `copies` sets: 4 = cache-resident like the diffusion head across
solver steps, many = streamed from HBM like the LLM.  The table switch (vv_tune "gemv_hot") is read when a launch is recorded, so one
graph per variant is captured and the variants are timed interleaved, REPS repetitions each.  A shape is adopted when the hot kernel's
worst repetition beats the generic kernel's best.

    python tools/mb_hot.py [out.txt]"""
import ctypes as C
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from vibevoice_rocm_amd import _lib as L

lib = L.load()
st = torch.cuda.Stream()
N_CHAIN, REPS, INNER = 240, 5, 5
REUSED = L.LIN_W_REUSED
#          name           bit  n     k     dual copies  operands
SHAPES = [("head.gate_up", 0, 4608, 1536, True, 4, dict(pro=1, mod=True, flags=REUSED)),
          ("head.down", 1, 1536, 4608, False, 4, dict(gate=True, res=True, flags=REUSED)),
          ("llm.gate_up", 2, 8960, 1536, True, 12, dict(pro=1)),
          ("llm.down", 3, 1536, 8960, False, 24, dict(res=True)),
          ("llm.qkv", 4, 2048, 1536, False, 64, dict(pro=1, bias=True)),
          ("llm.o", 5, 1536, 1536, False, 64, dict(res=True))]


def capture(n, k, dual, copies, hot, pro=0, mod=False, bias=False, gate=False, res=False, flags=0, m=2):
    lib.vv_tune(b"gemv_hot", hot)
    ld = max(n, k)
    keep = []
    t = lambda *a: torch.randn(*a, device="cuda")
    bufs = [t(m, ld) * 0.5 for _ in range(2)]
    keep += bufs
    ws = [((t(n, k) / k ** 0.5).bfloat16(), (t(n, k) / k ** 0.5).bfloat16() if dual else None) for _ in range(copies)]
    keep += [w for p in ws for w in p if w is not None]
    nw = torch.ones(k, device="cuda"); sh = torch.zeros(m, k, device="cuda"); sc = torch.zeros(m, k, device="cuda")
    bs = torch.zeros(n, device="cuda"); gt = torch.full((m, n), 0.5, device="cuda"); rs = torch.zeros(m, ld, device="cuda")
    keep += [nw, sh, sc, bs, gt, rs]
    L.check(lib.vv_graph_begin(st.cuda_stream), "begin")
    for i in range(N_CHAIN):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt = bufs[i & 1].data_ptr(), ld, m, n, k, L.VV_BF16
        a.out, a.ldo, a.flags = bufs[(i + 1) & 1].data_ptr(), ld, flags
        if pro == 1:
            a.pro, a.norm_w, a.eps = 1, nw.data_ptr(), 1e-5
        if mod:
            a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
        a.w = ws[i % copies][0].data_ptr()
        if dual:
            a.w2, a.act = ws[i % copies][1].data_ptr(), L.ACT_SWIGLU
        if bias:
            a.bias = bs.data_ptr()
        if gate:
            a.gate, a.gate_ld = gt.data_ptr(), n
        if res:
            a.res, a.ldres = rs.data_ptr(), ld
        L.check(lib.vv_linear(C.byref(a), st.cuda_stream), "vv_linear")
    ge = C.c_void_p()
    L.check(lib.vv_graph_end(st.cuda_stream, C.byref(ge)), "end")
    lib.vv_tune(b"gemv_hot", -1)
    return ge, keep


def one(ge):
    t0 = time.perf_counter()
    for _ in range(INNER):
        lib.vv_graph_launch(ge, st.cuda_stream)
    st.synchronize()
    return (time.perf_counter() - t0) / INNER / N_CHAIN * 1e6


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()

    say(f"# {torch.cuda.get_device_name(0)}; us per launch in a dependent graph chain of {N_CHAIN} launches, {REPS} repetitions of {INNER} replays, variants interleaved")
    say("# adopted: the hot kernel's worst repetition is faster than the generic kernel's best")
    with torch.cuda.stream(st):
        for name, bit, n, k, dual, copies, kw in SHAPES:
            variants = [("generic", 0), ("hot", 1 << bit)] + ([("hot rows3", (1 << bit) | 256)] if "down" in name else [])
            graphs = [(vn, *capture(n, k, dual, copies, hot, **kw)) for vn, hot in variants]
            st.synchronize()
            for _, ge, _k in graphs:
                for _ in range(3):
                    lib.vv_graph_launch(ge, st.cuda_stream)
            st.synchronize()
            times = {vn: [] for vn, _ in variants}
            for _ in range(REPS):
                for vn, ge, _k in graphs:
                    times[vn].append(one(ge))
            gen_best = min(times["generic"])
            for vn, _ in variants:
                ts = times[vn]
                verdict = "" if vn == "generic" else ("  ADOPT" if max(ts) < gen_best else "  keep generic")
                say(f"{name:13s} 2 x {n:4d} x {k:4d} {vn:10s} " + " ".join(f"{v:6.2f}" for v in ts) + f"   best {min(ts):6.2f} worst {max(ts):6.2f}{verdict}")
            for _, ge, _k in graphs:
                lib.vv_graph_destroy(ge)
            del graphs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
