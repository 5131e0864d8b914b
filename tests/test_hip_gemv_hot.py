"""The shape-specialised decode GEMVs (csrc/vv_gemv_hot.hip) against the generic weight-streaming template they replace for the six hot
1.5B matrices (M = 2, bf16 weights): bit for bit with the table switched on and off (vv_tune "gemv_hot"), eager and inside a captured graph;
each against torch fp64 on the bf16-rounded weights at the bar test_hip_parity.py::test_decode_gemv_vs_torch sets for the decode shapes
(relative RMS < 2e-5); calls one element off a table entry stay on the generic path and keep passing; and (no GPU) the table equals the
shapes that config.py's 1.5B preset gives, so a preset change cannot silently orphan it."""
import ctypes as C

import pytest
import torch

from conftest import rel_rms

DECODE_BAR = 2e-5          # tests/test_hip_parity.py::test_decode_gemv_vs_torch
ALL_ON = 0x3f              # every table entry on its hot kernel (the library's default is the adopted subset)
NAMES = ["head.gate_up", "head.down", "llm.gate_up", "llm.down", "llm.qkv", "llm.o"]


class HotShape(C.Structure):      # vv_gemv_hot_shape (csrc/vv_common.h)
    _fields_ = [("name", C.c_char_p)] + [(f, C.c_int) for f in ("m", "n", "k", "dual", "pro", "mod", "bias", "gate", "res", "act", "flags")]


def _table(lib):
    buf = (HotShape * 16)()
    lib.vv_gemv_hot_shapes.restype = C.c_int
    lib.vv_gemv_hot_shapes.argtypes = [C.POINTER(HotShape), C.c_int]
    n = lib.vv_gemv_hot_shapes(buf, 16)
    return [{f: getattr(buf[i], f) for f, _ in HotShape._fields_} for i in range(n)]


def test_table_equals_the_1p5b_preset_shapes():
    """The six entries are the head's and the LLM's per-frame matrices of the 1.5B preset, with the prologue / epilogue operands and the
    flags their call sites in csrc/vv_model.hip pass."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.config import VVConfig
    c = VVConfig.preset("1.5b")
    qkvd = (c.heads + 2 * c.kv_heads) * c.head_dim
    want = [
        dict(name=b"head.gate_up", m=2, n=c.head_ffn, k=c.head_hidden, dual=1, pro=L.PRO_RMSNORM, mod=1, bias=0, gate=0, res=0, act=L.ACT_SWIGLU, flags=L.LIN_W_REUSED),
        dict(name=b"head.down", m=2, n=c.head_hidden, k=c.head_ffn, dual=0, pro=L.PRO_NONE, mod=0, bias=0, gate=1, res=1, act=L.ACT_NONE, flags=L.LIN_W_REUSED),
        dict(name=b"llm.gate_up", m=2, n=c.inter, k=c.hidden, dual=1, pro=L.PRO_RMSNORM, mod=0, bias=0, gate=0, res=0, act=L.ACT_SWIGLU, flags=0),
        dict(name=b"llm.down", m=2, n=c.hidden, k=c.inter, dual=0, pro=L.PRO_NONE, mod=0, bias=0, gate=0, res=1, act=L.ACT_NONE, flags=0),
        dict(name=b"llm.qkv", m=2, n=qkvd, k=c.hidden, dual=0, pro=L.PRO_RMSNORM, mod=0, bias=1, gate=0, res=0, act=L.ACT_NONE, flags=0),
        dict(name=b"llm.o", m=2, n=c.hidden, k=c.heads * c.head_dim, dual=0, pro=L.PRO_NONE, mod=0, bias=0, gate=0, res=1, act=L.ACT_NONE, flags=0),
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
    yield _lib
    l.vv_tune(b"gemv_hot", -1)


class Call:
    """One vv_linear call with the operands of a table entry (seeded), its torch fp64 reference, and variations one element off."""

    def __init__(self, L, e, m=None, dn=0, dk=0, fp8=False):
        self.L, self.e = L, e
        m = e["m"] if m is None else m
        n, k = e["n"] + dn, e["k"] + dk
        self.m, self.n, self.k = m, n, k
        g = torch.Generator().manual_seed(e["n"] * 3 + e["k"] + m + dn + dk)
        r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
        x = r(m, k)
        w, w2 = (r(n, k) / k ** 0.5).bfloat16(), (r(n, k) / k ** 0.5).bfloat16()
        nw, sh, sc = 1 + r(k, sc=0.1), r(m, k, sc=0.2), r(m, k, sc=0.2)
        bias, gate, res = r(n, sc=0.1), r(m, n, sc=0.5), r(m, n)
        self.d = d = {kk: v.cuda().contiguous() for kk, v in dict(x=x, w=w, w2=w2, nw=nw, sh=sh, sc=sc, bias=bias, gate=gate, res=res).items()}
        a = self.a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.ldo = d["x"].data_ptr(), k, m, n, k, L.VV_BF16, n
        a.w, a.flags = d["w"].data_ptr(), e["flags"]
        xp = x.double()
        if e["pro"] == L.PRO_RMSNORM:
            a.pro, a.norm_w, a.eps = L.PRO_RMSNORM, d["nw"].data_ptr(), 1e-5
            xp = xp * torch.rsqrt((xp * xp).mean(-1, keepdim=True) + 1e-5) * nw.double()
            if e["mod"]:
                a.mod_shift, a.mod_scale, a.ld_mod = d["sh"].data_ptr(), d["sc"].data_ptr(), k
                xp = xp * (1 + sc.double()) + sh.double()
        wd, w2d = w.double(), w2.double()
        if fp8:      # e4m3fn codes + per-row scale: the generic kernel's fp8 instantiation
            self.q = [t.float().cuda().to(torch.float8_e4m3fn) for t in (w, w2)]
            self.qs = torch.ones(n, device="cuda")
            a.wdt, a.w, a.wscale = L.VV_FP8, self.q[0].data_ptr(), self.qs.data_ptr()
            wd, w2d = self.q[0].cpu().double(), self.q[1].cpu().double()
        y = xp @ wd.T
        if e["dual"]:
            a.w2, a.act = (self.q[1] if fp8 else d["w2"]).data_ptr(), L.ACT_SWIGLU
            if fp8:
                a.w2scale = self.qs.data_ptr()
            y = torch.nn.functional.silu(y) * (xp @ w2d.T)
        if e["bias"]:
            a.bias = d["bias"].data_ptr()
            y = y + bias.double()
        if e["gate"]:
            a.gate, a.gate_ld = d["gate"].data_ptr(), n
            y = y * gate.double()
        if e["res"]:
            a.res, a.ldres = d["res"].data_ptr(), n
            y = y + res.double()
        self.ref = y.float()

    def run(self, hot, graph=False):
        L, l = self.L, self.L.load()
        out = torch.full((self.m, self.n), float("nan"), device="cuda")
        self.a.out = out.data_ptr()
        L.check(l.vv_tune(b"gemv_hot", hot), "vv_tune")
        try:
            if not graph:
                L.check(l.vv_linear(C.byref(self.a), None), "vv_linear")
            else:
                st = torch.cuda.Stream()
                with torch.cuda.stream(st):
                    st.synchronize()
                    L.check(l.vv_graph_begin(st.cuda_stream), "begin")
                    L.check(l.vv_linear(C.byref(self.a), st.cuda_stream), "vv_linear")
                    ge = C.c_void_p()
                    L.check(l.vv_graph_end(st.cuda_stream, C.byref(ge)), "end")
                    L.check(l.vv_graph_launch(ge, st.cuda_stream), "launch")
                    st.synchronize()
                    l.vv_graph_destroy(ge)
            torch.cuda.synchronize()
        finally:
            l.vv_tune(b"gemv_hot", -1)
        return out


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(6), ids=NAMES)
@pytest.mark.parametrize("rows3", [0, 256], ids=["rows6", "rows3"])
def test_hot_equals_generic_bit_for_bit(lib, idx, rows3):
    """Table entry idx on its hot kernel (only its own bit set; bit 8: the down kernels' 3-rows-per-block variant) against the generic
    template (table off), same operands: torch.equal, eager and replayed from a captured graph."""
    e = _table(lib.load())[idx]
    if rows3 and "down" not in e["name"].decode():
        rows3 = 0              # bit 8 only changes the down kernels: the other entries run the same kernel in both cases
    c = Call(lib, e)
    ref = c.run(0)
    for graph in (False, True):
        got = c.run((1 << idx) | rows3, graph=graph)
        assert not torch.isnan(got).any()
        assert torch.equal(got, ref), f"{e['name'].decode()} graph={graph}: max |diff| {(got - ref).abs().max().item():.3e}"
    assert torch.equal(c.run(0, graph=True), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(6), ids=NAMES)
def test_hot_vs_torch_fp64(lib, idx):
    e = _table(lib.load())[idx]
    c = Call(lib, e)
    for hot in (ALL_ON, ALL_ON | 256):
        err = rel_rms(c.run(hot).cpu().numpy(), c.ref.numpy(), what=f"{e['name'].decode()} hot={hot:#x}")
        print(f"{e['name'].decode()} hot={hot:#x}: rel RMS vs fp64 {err:.3e} (bar {DECODE_BAR})")
        assert err < DECODE_BAR, f"{e['name'].decode()}: rel RMS {err:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(6), ids=NAMES)
@pytest.mark.parametrize("off", ["n+16", "k+32", "m=1", "m=3", "fp8"])
def test_one_off_the_table_takes_the_generic_path(lib, idx, off):
    """A call one element off an entry must not reach a hot kernel (which would compute the entry's shape): with every entry on it equals
    the table-off result bit for bit, and it stays inside the decode bar against fp64 (fp8: against the codes' own values)."""
    e = _table(lib.load())[idx]
    kw = {"n+16": dict(dn=16), "k+32": dict(dk=32), "m=1": dict(m=1), "m=3": dict(m=3), "fp8": dict(fp8=True)}[off]
    c = Call(lib, e, **kw)
    ref = c.run(0)
    got = c.run(ALL_ON)
    assert torch.equal(got, ref)
    err = rel_rms(got.cpu().numpy(), c.ref.numpy(), what=f"{e['name'].decode()} {off}")
    assert err < DECODE_BAR, f"{e['name'].decode()} {off}: rel RMS {err:.3e}"
