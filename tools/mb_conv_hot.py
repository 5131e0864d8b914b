"""Per-shape time of the conv tokenizers' one-row stage and hand-over GEMVs on today's kernels and on their own (csrc/vv_conv_hot.hip),
inside a hipGraph chain of 240 DEPENDENT launches on real operands (the pattern of mb_hot.py).  The three GEMV entries go through
vv_linear, x of launch i being the output of launch i - 1, the weights cycling through enough copies to come from HBM.  ffn_in_row is only
reachable through a convnet, so it is timed as the frame runs it: a one-stage streaming decoder with 8 one-row Block1D (8 x 67 MB of
weights) whose frame is stem conv, 8 x (ffn_in_row, W2 GEMV), head conv and the two state moves; 15 frames = 240 block launches, reported
per block pair (the 4 small launches around the blocks are in every variant alike).  The table switch (vv_tune "conv_hot") is read when
a launch is recorded, so one graph per variant is captured and the variants are timed interleaved, REPS repetitions each.  An entry is
adopted when its hot kernel's worst repetition beats today's best.

    python tools/mb_conv_hot.py [out.txt]"""
import ctypes as C
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from vibevoice_rocm_amd import _lib as L

lib = L.load()
L.check(lib.vv_init(), "vv_init")
st = torch.cuda.Stream()
N_CHAIN, REPS, INNER = 240, 5, 5
ALT, NT = 256, 512
#          name          bit  n     k      copies operands
GEMVS = [("block.w2", 0, 2048, 8192, 16, dict(gate=True, res=True)),
         ("dec.handover", 2, 8192, 4096, 8, dict()),
         ("sem.handover", 3, 2048, 16384, 8, dict())]


def capture_gemv(n, k, copies, hot, gate=False, res=False):
    lib.vv_tune(b"conv_hot", hot)
    ld = max(n, k)
    t = lambda *a: torch.randn(*a, device="cuda")
    bufs = [t(1, ld) * 0.5 for _ in range(2)]
    ws = [(t(n, k) / k ** 0.5).bfloat16() for _ in range(copies)]
    bs = torch.zeros(n, device="cuda"); gt = torch.full((n,), 0.5, device="cuda"); rs = torch.zeros(1, ld, device="cuda")
    keep = bufs + ws + [bs, gt, rs]
    L.check(lib.vv_graph_begin(st.cuda_stream), "begin")
    for i in range(N_CHAIN):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt = bufs[i & 1].data_ptr(), ld, 1, n, k, L.VV_BF16
        a.out, a.ldo = bufs[(i + 1) & 1].data_ptr(), ld
        a.w, a.bias = ws[i % copies].data_ptr(), bs.data_ptr()
        if gate:
            a.gate, a.gate_ld = gt.data_ptr(), 0
        if res:
            a.res, a.ldres = rs.data_ptr(), ld
        L.check(lib.vv_linear(C.byref(a), st.cuda_stream), "vv_linear")
    ge = C.c_void_p()
    L.check(lib.vv_graph_end(st.cuda_stream, C.byref(ge)), "end")
    lib.vv_tune(b"conv_hot", -1)
    return ge, keep


class RowNet:
    """One-stage streaming decoder at the one-row shape (C = 2048): stem conv 64 -> C (kernel 7), NB Block1D, kernel-1 head conv C -> 64."""

    def __init__(self, nb=8, Cc=2048, lat=64):
        t = lambda *a, sc=1.0: torch.randn(*a, device="cuda") * sc
        self.keep = keep = []
        dev = lambda x: keep.append(x.contiguous()) or keep[-1]
        net = self.net = L.ConvNet()
        net.wdt, net.n_stages, net.eps = L.VV_BF16, 1, 1e-5
        cv = net.sample[0]
        cv.w, cv.b = dev((t(Cc, 7 * lat) / (7 * lat) ** 0.5).bfloat16()).data_ptr(), dev(t(Cc, sc=0.1)).data_ptr()
        cv.cin, cv.cout, cv.kk, cv.stride, cv.transposed, cv.state = lat, Cc, 7, 1, 0, dev(torch.zeros(6, lat, device="cuda")).data_ptr()
        self.arr = arr = (L.Block * nb)()
        for j in range(nb):
            B = arr[j]
            dw = dev(t(Cc, 7, sc=0.3))
            B.gamma, B.ffn_gamma, B.norm_w, B.ffn_norm_w = (dev(v).data_ptr() for v in (t(Cc, sc=0.1), t(Cc, sc=0.1), 1 + t(Cc, sc=0.1), 1 + t(Cc, sc=0.1)))
            B.dw_w, B.dw_b, B.dw_last = dw.data_ptr(), dev(t(Cc, sc=0.1)).data_ptr(), dev(dw[:, 6]).data_ptr()
            B.w1, B.b1 = dev((t(4 * Cc, Cc) / Cc ** 0.5).bfloat16()).data_ptr(), dev(t(4 * Cc, sc=0.1)).data_ptr()
            B.w2, B.b2 = dev((t(Cc, 4 * Cc) / (4 * Cc) ** 0.5).bfloat16()).data_ptr(), dev(t(Cc, sc=0.1)).data_ptr()
            B.hist, B.hs = dev(torch.zeros(6, Cc, device="cuda")).data_ptr(), dev(torch.zeros(Cc, device="cuda")).data_ptr()
        net.n_blocks[0] = nb
        net.blocks[0] = C.cast(arr, C.POINTER(L.Block))
        hd = net.head
        hd.w, hd.b = dev((t(lat, Cc) / Cc ** 0.5).bfloat16()).data_ptr(), dev(t(lat, sc=0.1)).data_ptr()
        hd.cin, hd.cout, hd.kk, hd.stride, hd.transposed, hd.state = Cc, lat, 1, 1, 0, None
        self.ws = dev(torch.empty(lib.vv_convnet_ws_bytes(C.byref(net), 1, 1), dtype=torch.uint8, device="cuda"))
        self.lat = [dev(t(1, lat)) for _ in range(2)]          # frame i reads the "waveform" row frame i - 1 wrote: a dependent chain
        self.nb = nb

    def capture(self, hot):
        lib.vv_tune(b"conv_hot", hot)
        L.check(lib.vv_graph_begin(st.cuda_stream), "begin")
        for i in range(N_CHAIN // (2 * self.nb)):
            L.check(lib.vv_decoder_forward(C.byref(self.net), self.lat[i & 1].data_ptr(), 1, 1.0, 0.0, self.lat[(i + 1) & 1].data_ptr(), self.ws.data_ptr(),
                                           st.cuda_stream), "dec")
        ge = C.c_void_p()
        L.check(lib.vv_graph_end(st.cuda_stream, C.byref(ge)), "end")
        lib.vv_tune(b"conv_hot", -1)
        return ge


def one(ge, per):
    t0 = time.perf_counter()
    for _ in range(INNER):
        lib.vv_graph_launch(ge, st.cuda_stream)
    st.synchronize()
    return (time.perf_counter() - t0) / INNER / per * 1e6


def race(say, label, graphs, per, base="generic"):
    st.synchronize()
    for _, ge in graphs:
        for _ in range(3):
            lib.vv_graph_launch(ge, st.cuda_stream)
    st.synchronize()
    times = {vn: [] for vn, _ in graphs}
    for _ in range(REPS):
        for vn, ge in graphs:
            times[vn].append(one(ge, per))
    best = min(times[base])
    for vn, _ in graphs:
        ts = times[vn]
        verdict = "" if vn == base else ("  ADOPT" if max(ts) < best else "  keep generic")
        say(f"{label:28s} {vn:18s} " + " ".join(f"{v:6.2f}" for v in ts) + f"   best {min(ts):6.2f} worst {max(ts):6.2f}{verdict}")
    for _, ge in graphs:
        lib.vv_graph_destroy(ge)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n"); out.flush()

    say(f"# {torch.cuda.get_device_name(0)}; us per launch (GEMVs) or per block pair ffn_in_row + W2 (one-row stage) in a dependent graph chain of {N_CHAIN} "
        f"launches, {REPS} repetitions of {INNER} replays, variants interleaved")
    say("# adopted: the hot kernel's worst repetition is faster than today's best")
    with torch.cuda.stream(st):
        for name, bit, n, k, copies, kw in GEMVS:
            keeps, graphs = [], []
            for vn, hot in (("generic", 0), ("hot", 1 << bit), ("hot other rows", (1 << bit) | ALT)):
                ge, keep = capture_gemv(n, k, copies, hot, **kw)
                graphs.append((vn, ge)); keeps.append(keep)
            race(say, f"{name} 1 x {n} x {k}", graphs, N_CHAIN)
            del keeps, graphs
            torch.cuda.empty_cache()
        net = RowNet()
        variants = (("generic", 0), ("hot w2", 1), ("hot row", 2), ("hot row nt", 2 | NT), ("hot row + w2", 3), ("hot row + w2 other", 3 | ALT))
        race(say, "one-row block (row + w2)", [(vn, net.capture(hot)) for vn, hot in variants], (N_CHAIN // (2 * net.nb)) * net.nb)


if __name__ == "__main__":
    main()
