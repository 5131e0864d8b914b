"""The conv tokenizers' shape-specialised kernels (csrc/vv_conv_hot.hip) against the paths they replace: the one-row Block1D's W2 GEMV and
the two hand-over GEMVs against the generic weight-streaming template (through vv_linear), the one-row block's first FFN half against
ffn_in_row_kernel (through vv_decoder_forward on a one-stage streaming net at the real C = 2048).  Bit for bit with the table switched on
and off (vv_tune "conv_hot"), eager and replayed from a captured graph; each against torch fp64 so that a shared bug cannot hide behind
the equality (GEMVs: relative RMS < 2e-5, the bar of test_hip_gemv_hot.py; the one-row stage: < 2e-2, the bf16 bar of
test_hip_realshape.py::test_one_row_stage_state_paths_1p5b_vs_oracle); calls one element off a table entry stay on today's path; and
(no GPU) the table equals the shapes config.py's presets give the tokenizers."""
import ctypes as C

import pytest
import torch

from conftest import rel_rms

GEMV_BAR = 2e-5            # tests/test_hip_gemv_hot.py (test_hip_parity.py::test_decode_gemv_vs_torch)
ROW_BAR = 2e-2             # tests/test_hip_realshape.py::test_one_row_stage_state_paths_1p5b_vs_oracle
ALL_ON = 0xf               # every table entry on its hot kernel (the library's default is the adopted subset)
ALT = 256                  # bit 8: the GEMVs on their other rows-per-block choice
NT = 512                   # bit 9: ffn_in_row's W1 with non-temporal loads
NAMES = ["block.w2", "block.ffn_in_row", "dec.handover", "sem.handover"]
GEMV, ROW = 0, 1
GEMV_IDX = [0, 2, 3]


class HotShape(C.Structure):      # vv_conv_hot_shape (include/vv_hip.h)
    _fields_ = [("name", C.c_char_p)] + [(f, C.c_int) for f in ("kind", "m", "n", "k", "bias", "gate", "res")]


def _table(lib):
    buf = (HotShape * 16)()
    n = lib.vv_conv_hot_shapes(C.cast(buf, C.c_void_p), 16)
    return [{f: getattr(buf[i], f) for f, _ in HotShape._fields_} for i in range(n)]


@pytest.mark.parametrize("preset", ["1.5b", "7b"])
def test_table_equals_the_preset_tokenizer_shapes(preset):
    """The four entries are the one-row stage (C = filters * 2 ** len(ratios)) of both tokenizers and the convs next to it, as their call
    sites in csrc/vv_model.hip build them; the 7B preset's tokenizers are the 1.5B's."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.config import VVConfig
    c = VVConfig.preset(preset)
    assert (c.ac_filters, c.ac_dec_filters, c.ac_ratios) == (c.sem_filters, c.ac_filters, c.sem_ratios)
    top = c.ac_filters * 2 ** len(c.ac_ratios)
    s = c.ac_ratios[0]                       # the resampling conv next to the one-row stage: stride s, kernel 2 s, top / 2 channels on the far side
    want = [
        dict(name=b"block.w2", kind=GEMV, m=1, n=top, k=4 * top, bias=1, gate=1, res=1),
        dict(name=b"block.ffn_in_row", kind=ROW, m=1, n=4 * top, k=top, bias=1, gate=0, res=0),
        dict(name=b"dec.handover", kind=GEMV, m=1, n=s * (top // 2), k=2 * top, bias=1, gate=0, res=0),
        dict(name=b"sem.handover", kind=GEMV, m=1, n=top, k=2 * s * (top // 2), bias=1, gate=0, res=0),
    ]
    assert [w["name"].decode() for w in want] == NAMES
    assert _table(L.load()) == want


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib
    l = _lib.load()
    _lib.check(l.vv_init(), "vv_init")
    yield _lib
    l.vv_tune(b"conv_hot", -1)


def _graphed(L, l, st, fn):
    """fn() recorded into a graph on stream st; returns the executable graph."""
    st.synchronize()
    L.check(l.vv_graph_begin(st.cuda_stream), "begin")
    fn()
    ge = C.c_void_p()
    L.check(l.vv_graph_end(st.cuda_stream, C.byref(ge)), "end")
    return ge


class Call:
    """One vv_linear call with the operands of a GEMV table entry (seeded), its torch fp64 reference, and variations one element off."""

    def __init__(self, L, e, m=None, dn=0, dk=0, fp8=False, gate_rows=False):
        self.L = L
        m = e["m"] if m is None else m
        n, k = e["n"] + dn, e["k"] + dk
        self.m, self.n, self.k = m, n, k
        g = torch.Generator().manual_seed(e["n"] * 3 + e["k"] + m + dn + dk)
        r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
        x = r(m, k)
        w = (r(n, k) / k ** 0.5).bfloat16()
        bias, gate, res = r(n, sc=0.1), r(m if gate_rows else 1, n, sc=0.5), r(m, n)
        self.d = d = {kk: v.cuda().contiguous() for kk, v in dict(x=x, w=w, bias=bias, gate=gate, res=res).items()}
        a = self.a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.ldo = d["x"].data_ptr(), k, m, n, k, L.VV_BF16, n
        a.w = d["w"].data_ptr()
        wd = w.double()
        if fp8:      # what a q_w2 companion turns the call into: e4m3fn codes + per-row scale (the generic kernel's fp8 instantiation)
            self.q = w.float().cuda().to(torch.float8_e4m3fn)
            self.qs = torch.ones(n, device="cuda")
            a.wdt, a.w, a.wscale = L.VV_FP8, self.q.data_ptr(), self.qs.data_ptr()
            wd = self.q.cpu().double()
        y = x.double() @ wd.T
        if e["bias"]:
            a.bias = d["bias"].data_ptr()
            y = y + bias.double()
        if e["gate"]:
            a.gate, a.gate_ld = d["gate"].data_ptr(), (n if gate_rows else 0)
            y = y * gate.double()
        if e["res"]:
            a.res, a.ldres = d["res"].data_ptr(), n
            y = y + res.double()
        self.ref = y.float()

    def run(self, hot, graph=False):
        L, l = self.L, self.L.load()
        out = torch.full((self.m, self.n), float("nan"), device="cuda")
        self.a.out = out.data_ptr()
        L.check(l.vv_tune(b"conv_hot", hot), "vv_tune")
        try:
            if not graph:
                L.check(l.vv_linear(C.byref(self.a), None), "vv_linear")
            else:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    ge = _graphed(L, l, st, lambda: L.check(l.vv_linear(C.byref(self.a), st.cuda_stream), "vv_linear"))
                    L.check(l.vv_graph_launch(ge, st.cuda_stream), "launch")
                    st.synchronize()
                    l.vv_graph_destroy(ge)
            torch.cuda.synchronize()
        finally:
            l.vv_tune(b"conv_hot", -1)
        return out


@pytest.mark.gpu
@pytest.mark.parametrize("idx", GEMV_IDX, ids=[NAMES[i] for i in GEMV_IDX])
@pytest.mark.parametrize("alt", [0, ALT], ids=["rows", "other_rows"])
def test_hot_gemv_equals_generic_bit_for_bit(lib, idx, alt):
    """GEMV entry idx on its hot kernel (only its own bit set; bit 8: the other rows-per-block choice) against the generic template (table off),
    same operands: torch.equal, eager and replayed from a captured graph."""
    e = _table(lib.load())[idx]
    c = Call(lib, e)
    ref = c.run(0)
    assert not torch.isnan(ref).any()
    for graph in (False, True):
        got = c.run((1 << idx) | alt, graph=graph)
        assert not torch.isnan(got).any()
        assert torch.equal(got, ref), f"{e['name'].decode()} graph={graph}: max |diff| {(got - ref).abs().max().item():.3e}"
    assert torch.equal(c.run(0, graph=True), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", GEMV_IDX, ids=[NAMES[i] for i in GEMV_IDX])
def test_hot_gemv_vs_torch_fp64(lib, idx):
    e = _table(lib.load())[idx]
    c = Call(lib, e)
    for hot in (ALL_ON, ALL_ON | ALT):
        err = rel_rms(c.run(hot).cpu().numpy(), c.ref.numpy(), what=f"{e['name'].decode()} hot={hot:#x}")
        print(f"{e['name'].decode()} hot={hot:#x}: rel RMS vs fp64 {err:.3e} (bar {GEMV_BAR})")
        assert err < GEMV_BAR, f"{e['name'].decode()}: rel RMS {err:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("idx", GEMV_IDX, ids=[NAMES[i] for i in GEMV_IDX])
@pytest.mark.parametrize("off", ["n+16", "k+32", "m=2", "q_w2", "gate_ld"])
def test_one_off_the_table_takes_the_generic_path(lib, idx, off):
    """A call one element off an entry must not reach a hot kernel (which would compute the entry's shape): with every entry on it equals
    the table-off result bit for bit, and it stays inside the GEMV bar against fp64 (q_w2, the fp8 companion of a one-row block's W2:
    against the codes' own values).  gate_ld != 0 (a gate row per activation row) only exists for the entry that has a gate."""
    e = _table(lib.load())[idx]
    if off == "gate_ld" and not e["gate"]:
        e = dict(e, gate=1)            # the entry's shape with a per-row gate added: also off the table
    kw = {"n+16": dict(dn=16), "k+32": dict(dk=32), "m=2": dict(m=2), "q_w2": dict(fp8=True), "gate_ld": dict(gate_rows=True)}[off]
    c = Call(lib, e, **kw)
    ref = c.run(0)
    got = c.run(ALL_ON)
    assert torch.equal(got, ref)
    err = rel_rms(got.cpu().numpy(), c.ref.numpy(), what=f"{e['name'].decode()} {off}")
    assert err < GEMV_BAR, f"{e['name'].decode()} {off}: rel RMS {err:.3e}"


# ---- the one-row stage through vv_decoder_forward ------------------------------------------------------------------------------------

class RowNet:
    """A one-stage streaming decoder at the real one-row shape: stem conv (latent 64 -> C = 2048, kernel 7), NB one-row Block1D, and a
    kernel-1 head conv whose weight is the identity, so `wav` is the last block's output row exactly (x * 1.0 + zeros in fp32).  With
    ffn_gamma = 0 in the last block that row is the block's mixer output y (0 * (W2 h + b2) + y); the new history rows and hs are read
    from the net's state tensors; `hidden` reaches the output through W2."""
    C_, LAT, NB, EPS = 2048, 64, 2, 1e-5

    def __init__(self, L, y_only=False):
        self.L = L
        Cc, lat = self.C_, self.LAT
        g = torch.Generator().manual_seed(2048 + int(y_only))
        r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
        self.keep = []
        dev = lambda t: self.keep.append(t.cuda().contiguous()) or self.keep[-1]
        self.p = p = dict(stem_w=(r(Cc, 7 * lat) / (7 * lat) ** 0.5).bfloat16(), stem_b=r(Cc, sc=0.1), blocks=[])
        net = self.net = L.ConvNet()
        net.wdt, net.n_stages, net.eps = L.VV_BF16, 1, self.EPS
        self.stem_state = torch.zeros(6, lat, device="cuda")
        cv = net.sample[0]
        cv.w, cv.b, cv.cin, cv.cout, cv.kk, cv.stride, cv.transposed = dev(p["stem_w"]).data_ptr(), dev(p["stem_b"]).data_ptr(), lat, Cc, 7, 1, 0
        cv.state = self.stem_state.data_ptr()
        self.arr = arr = (L.Block * self.NB)()
        self.hist, self.hs = [], []
        for j in range(self.NB):
            b = dict(gamma=r(Cc, sc=0.5), ffn_gamma=r(Cc, sc=0.5), norm_w=1 + r(Cc, sc=0.1), ffn_norm_w=1 + r(Cc, sc=0.1), dw_w=r(Cc, 7, sc=0.3),
                     dw_b=r(Cc, sc=0.1), w1=(r(4 * Cc, Cc) / Cc ** 0.5).bfloat16(), b1=r(4 * Cc, sc=0.1),
                     w2=(r(Cc, 4 * Cc) / (4 * Cc) ** 0.5).bfloat16(), b2=r(Cc, sc=0.1))
            if y_only and j == self.NB - 1:
                b["ffn_gamma"] = torch.zeros(Cc)
            p["blocks"].append(b)
            B = arr[j]
            for kk in ("gamma", "ffn_gamma", "norm_w", "ffn_norm_w", "dw_w", "dw_b", "w1", "b1", "w2", "b2"):
                setattr(B, kk, dev(b[kk]).data_ptr())
            B.dw_last = dev(b["dw_w"][:, 6]).data_ptr()
            self.hist.append(torch.zeros(6, Cc, device="cuda"))
            self.hs.append(torch.zeros(Cc, device="cuda"))
            B.hist, B.hs = self.hist[-1].data_ptr(), self.hs[-1].data_ptr()
        net.n_blocks[0] = self.NB
        net.blocks[0] = C.cast(arr, C.POINTER(L.Block))
        hd = net.head
        hd.w, hd.b = dev(torch.eye(Cc).bfloat16()).data_ptr(), dev(torch.zeros(Cc)).data_ptr()
        hd.cin, hd.cout, hd.kk, hd.stride, hd.transposed, hd.state = Cc, Cc, 1, 1, 0, None
        l = L.load()
        self.ws = torch.empty(l.vv_convnet_ws_bytes(C.byref(net), 1, 1), dtype=torch.uint8, device="cuda")
        self.lats = [r(1, lat) for _ in range(2)]

    def reset(self):
        for t in [self.stem_state] + self.hist + self.hs:
            t.zero_()

    def run(self, hot, graph=False):
        """Two consecutive frames from zeroed state; returns per frame (out row, [hist per block], [hs per block])."""
        L, l = self.L, self.L.load()
        st = torch.cuda.Stream()
        lat = torch.empty(1, self.LAT, device="cuda")
        wav = torch.full((self.C_,), float("nan"), device="cuda")
        frames = []
        with torch.cuda.stream(st):
            self.reset()
            fwd = lambda: L.check(l.vv_decoder_forward(C.byref(self.net), lat.data_ptr(), 1, 1.0, 0.0, wav.data_ptr(), self.ws.data_ptr(), st.cuda_stream), "dec")
            L.check(l.vv_tune(b"conv_hot", hot), "vv_tune")
            try:
                ge = _graphed(L, l, st, fwd) if graph else None
                for f in range(2):
                    lat.copy_(self.lats[f])
                    if graph:
                        L.check(l.vv_graph_launch(ge, st.cuda_stream), "launch")
                    else:
                        fwd()
                    st.synchronize()
                    frames.append((wav.clone(), [h.clone() for h in self.hist], [h.clone() for h in self.hs]))
                if graph:
                    l.vv_graph_destroy(ge)
            finally:
                l.vv_tune(b"conv_hot", -1)
        return frames

    def reference(self):
        """The same two frames in torch fp64 (Block1D.forward, modular_vibevoice_tokenizer.py:555-600, one row per call)."""
        p, eps = self.p, self.EPS
        rms = lambda v, w: v * torch.rsqrt((v * v).mean() + eps) * w.double()
        stem_hist = torch.zeros(6, self.LAT, dtype=torch.float64)
        hists = [torch.zeros(6, self.C_, dtype=torch.float64) for _ in range(self.NB)]
        out = []
        for f in range(2):
            win = torch.cat([stem_hist, self.lats[f].double()])                     # [7, lat]
            stem_hist = win[1:]
            x = p["stem_w"].double() @ win.reshape(-1) + p["stem_b"].double()
            for j, b in enumerate(p["blocks"]):
                xn = rms(x, b["norm_w"])
                win = torch.cat([hists[j], xn[None]])                               # [7, C]
                hists[j] = win[1:]
                conv = (b["dw_w"].double().t() * win).sum(0) + b["dw_b"].double()
                y = x + b["gamma"].double() * conv
                h = torch.nn.functional.gelu(b["w1"].double() @ rms(y, b["ffn_norm_w"]) + b["b1"].double())
                x = y + b["ffn_gamma"].double() * (b["w2"].double() @ h + b["b2"].double())
            hs = [(b["dw_w"].double()[:, :6].t() * hists[j]).sum(0) for j, b in enumerate(p["blocks"])]
            out.append((x.float(), [h.float() for h in hists], [h.float() for h in hs]))
        return out


def _same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[1] + a[2], b[1] + b[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("y_only", [False, True], ids=["out", "y"])
def test_hot_row_equals_ffn_in_row_bit_for_bit(lib, y_only):
    """ffn_in_row on its hot kernel (bit 1 alone, with non-temporal W1 loads, and next to the hot W2) against today's kernel, two consecutive
    frames so that the second reads the hs the closing scatter refreshed from the first's history rows: the block output (y_only: the
    mixer output y itself), every block's new history rows and hs, torch.equal, eager and replayed from a captured graph."""
    net = RowNet(lib, y_only)
    ref = net.run(0)
    for f in ref:
        assert not torch.isnan(f[0]).any() and float(f[1][0].abs().max()) > 0 and float(f[0].abs().max()) > 0
    assert float(ref[1][2][0].abs().max()) > 0, "hs stayed zero: the second frame would not cover its refresh"
    for hot in (2, 2 | NT, 3, ALL_ON | ALT):
        for graph in (False, True):
            got = net.run(hot, graph=graph)
            for f in range(2):
                assert _same(got[f], ref[f]), f"conv_hot={hot:#x} graph={graph} frame {f}: max |diff| of the output row {(got[f][0] - ref[f][0]).abs().max().item():.3e}"
    again = net.run(0, graph=True)
    assert all(_same(again[f], ref[f]) for f in range(2))


@pytest.mark.gpu
def test_hot_row_vs_torch_fp64(lib):
    net = RowNet(lib)
    want = net.reference()
    for hot in (0, ALL_ON):
        got = net.run(hot)
        for f in range(2):
            errs = [rel_rms(got[f][0].cpu().numpy(), want[f][0].numpy(), what=f"frame {f} out")]
            errs += [rel_rms(g.cpu().numpy(), w.numpy(), what=f"frame {f} state") for g, w in zip(got[f][1] + got[f][2], want[f][1] + want[f][2])]
            print(f"conv_hot={hot:#x} frame {f}: rel RMS vs fp64: out {errs[0]:.3e}, states max {max(errs[1:]):.3e} (bar {ROW_BAR})")
            assert max(errs) < ROW_BAR, f"conv_hot={hot:#x} frame {f}: rel RMS {max(errs):.3e}"
