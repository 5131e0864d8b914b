"""Kernarg preload on the hot decode GEMVs (csrc/vv_gemv_hot.hip): their leading arguments reach a wave in user SGPRs, so its first
instructions are global_loads instead of a scalar round trip to the kernarg segment.

No GPU: the kernel descriptors of the gfx950 code object inside the built library say which kernels preload and how many dwords (the low 7
bits of the 16-bit field at byte 58 of `<symbol>.kd`); the set must equal PRELOAD below, and every length must cover the leading dwords the
kernel's first loads need.  That fails when the build flag is dropped, and when a struct moves back in front of a kernel's pointers.

GPU: argument passing cannot change a result, so every table entry is compared with torch.equal against the generic template (vv_tune
"gemv_hot" 0) on operands that expose a swapped, dropped or truncated argument: every stride different and larger than its row, every operand
at its own non-zero offset of one allocation, NaN around every output row, two rows of different contents; eager and replayed from a captured
graph.  A call whose stride does not fit the kernels' 32-bit stride arguments must be routed to the template (vv_linear_route; nothing is
dereferenced)."""
import ctypes as C
import struct

import pytest
import torch

# mangled-name fragment of every kernel that preloads -> the dwords its loads in front of the first wait need (pointers 2, strides 1 each)
PRELOAD = {
    "15hot_dual_kernelILi4608ELb1ELb0EE": 14,        # head.gate_up: x, norm_w, mod_shift, mod_scale, w, w2, ldx, ld_mod
    "15hot_dual_kernelILi8960ELb0ELb1EE": 14,        # llm.gate_up
    "15hot_down_kernelILi1536ELi4608ELi6ELb1ELb0EE": 11,   # head.down: x, gate, res, w, ldx, gate_ld, ldres
    "15hot_down_kernelILi1536ELi4608ELi3ELb1ELb0EE": 11,   # its 3-rows-per-block variant (vv_tune "gemv_hot" bit 8)
    "15hot_down_kernelILi1536ELi8960ELi6ELb0ELb1EE": 11,   # llm.down
    "15hot_down_kernelILi1536ELi8960ELi3ELb0ELb1EE": 11,
    "15hot_rows_kernelILi2048ELi4ELb1ELb1EE": 10,    # llm.qkv: x, norm_w, bias, w, ldx, (ldres)
    "15hot_rows_kernelILi1536ELi3ELb0ELb1EE": 10,    # llm.o: x, (norm_w), res, w, ldx, ldres
}
NAMES = ["head.gate_up", "head.down", "llm.gate_up", "llm.down", "llm.qkv", "llm.o"]
BUNDLE = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(blob):
    """The gfx950 ELF images of every offload bundle in the library."""
    at = blob.find(BUNDLE)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(BUNDLE))
        p = at + len(BUNDLE) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl]
            p += 24 + tl
            if size and b"gfx950" in triple:
                yield blob[at + off:at + off + size]
        at = blob.find(BUNDLE, at + 1)


def _kernel_descriptors(elf):
    """{symbol without .kd: its 64 descriptor bytes} of one ELF64 little-endian code object."""
    assert elf[:6] == b"\x7fELF\x02\x01"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr offset size link info align entsize
    out = {}
    for sec in secs:
        if sec[1] != 2:          # SHT_SYMTAB
            continue
        stroff = secs[sec[6]][4]
        for o in range(sec[4], sec[4] + sec[5], 24):
            name_o, _info, _other, shndx, value, size = struct.unpack_from("<IBBHQQ", elf, o)
            end = elf.index(b"\0", stroff + name_o)
            name = elf[stroff + name_o:end].decode()
            if name.endswith(".kd") and size == 64 and 0 < shndx < shnum:
                home = secs[shndx]
                fo = home[4] + (value - home[3])
                out[name[:-3]] = elf[fo:fo + 64]
    return out


def _preload_lengths():
    from vibevoice_rocm_amd import build
    blob = open(build.OUT, "rb").read()
    kds = {}
    for elf in _code_objects(blob):
        kds.update(_kernel_descriptors(elf))
    assert kds, "no gfx950 kernel descriptor found in the built library"
    return {name: struct.unpack_from("<H", kd, 58)[0] & 0x7F for name, kd in kds.items()}


def test_preloading_kernels_are_the_table_and_cover_their_leading_arguments():
    lengths = _preload_lengths()
    assert len(lengths) > 100            # the whole library was read, not one unit
    have = {name: n for name, n in lengths.items() if n > 0}
    for frag, need in PRELOAD.items():
        hit = [name for name in have if frag in name]
        assert len(hit) == 1, f"{frag}: kernels that preload: {hit}"
        assert have[hit[0]] >= need, f"{hit[0]} preloads {have[hit[0]]} dwords, its first loads need {need}"
    extra = [name for name in have if not any(frag in name for frag in PRELOAD)]
    assert not extra, f"kernels that preload without an entry in the table: {extra}"


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib
    l = _lib.load()
    yield _lib
    l.vv_tune(b"gemv_hot", -1)


class HotShape(C.Structure):      # vv_gemv_hot_shape (csrc/vv_common.h)
    _fields_ = [("name", C.c_char_p)] + [(f, C.c_int) for f in ("m", "n", "k", "dual", "pro", "mod", "bias", "gate", "res", "act", "flags")]


def _table(L):
    l = L.load()
    buf = (HotShape * 16)()
    l.vv_gemv_hot_shapes.restype = C.c_int
    l.vv_gemv_hot_shapes.argtypes = [C.POINTER(HotShape), C.c_int]
    n = l.vv_gemv_hot_shapes(buf, 16)
    return [{f: getattr(buf[i], f) for f, _ in HotShape._fields_} for i in range(n)]


_CARVED = {}


def _carved(L, idx):
    """One set of operands per entry, shared by the tests (run() restores the pristine image first)."""
    if idx not in _CARVED:
        _CARVED[idx] = Carved(L, _table(L)[idx])
    return _CARVED[idx]


class Carved:
    """A table entry's operands carved out of ONE allocation, each at its own non-zero 16-byte-aligned offset, every stride different and
    larger than the row it strides over, the allocation NaN wherever no operand lives (so the output rows are fenced by NaN)."""

    def __init__(self, L, e):
        self.L, self.e = L, e
        m, n, k = e["m"], e["n"], e["k"]
        self.m, self.n = m, n
        self.ldx, self.ld_mod, self.gate_ld, self.ldres, self.ldo = k + 8, k + 12, n + 16, n + 24, n + 32
        g = torch.Generator().manual_seed(7 * n + k)
        r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
        f32 = dict(x=(r(m, k), self.ldx), nw=(1 + r(1, k, sc=0.1), k), sh=(r(m, k, sc=0.2), self.ld_mod), sc=(r(m, k, sc=0.2), self.ld_mod),
                   bias=(r(1, n, sc=0.1), n), gate=(r(m, n, sc=0.5), self.gate_ld), res=(r(m, n), self.ldres), out=(torch.full((m, n), float("nan")), self.ldo))
        assert not torch.equal(f32["x"][0][0], f32["x"][0][1])
        w = [(r(n, k) / k ** 0.5).bfloat16() for _ in range(2)]
        total = sum(4 + rows.shape[0] * ld for rows, ld in f32.values()) + 2 * (n * k // 2 + 4) + 4
        self.buf = torch.full((total,), float("nan"), device="cuda")
        self.at, at = {}, 4                      # offsets in floats: multiples of 4 (16 bytes), never 0
        for name, (rows, ld) in f32.items():
            self.at[name] = at
            view = self.buf[at:at + rows.shape[0] * ld].view(rows.shape[0], ld)
            view[:, :rows.shape[1]] = rows.cuda()
            at += rows.shape[0] * ld + 4
            at += -at % 4
        for name, t in zip(("w", "w2"), w):
            self.at[name] = at
            self.buf[at:at + n * k // 2].view(torch.bfloat16).copy_(t.cuda().reshape(-1))
            at += n * k // 2 + 4
        assert at <= total
        self.image = self.buf.clone()            # the allocation before any launch

    def ptr(self, name):
        return self.buf.data_ptr() + 4 * self.at[name]

    def args(self):
        L, e = self.L, self.e
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt = self.ptr("x"), self.ldx, e["m"], e["n"], e["k"], L.VV_BF16
        a.w, a.flags, a.out, a.ldo, a.act = self.ptr("w"), e["flags"], self.ptr("out"), self.ldo, e["act"]
        if e["pro"] == L.PRO_RMSNORM:
            a.pro, a.norm_w, a.eps = L.PRO_RMSNORM, self.ptr("nw"), 1e-5
        if e["mod"]:
            a.mod_shift, a.mod_scale, a.ld_mod = self.ptr("sh"), self.ptr("sc"), self.ld_mod
        if e["dual"]:
            a.w2 = self.ptr("w2")
        if e["bias"]:
            a.bias = self.ptr("bias")
        if e["gate"]:
            a.gate, a.gate_ld = self.ptr("gate"), self.gate_ld
        if e["res"]:
            a.res, a.ldres = self.ptr("res"), self.ldres
        return a

    def run(self, hot, graph=False):
        """The whole allocation after one launch from its pristine image."""
        L, l = self.L, self.L.load()
        self.buf.copy_(self.image)
        a = self.args()
        L.check(l.vv_tune(b"gemv_hot", hot), "vv_tune")
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                torch.cuda.synchronize()
                if not graph:
                    L.check(l.vv_linear(C.byref(a), st.cuda_stream), "vv_linear")
                else:
                    L.check(l.vv_graph_begin(st.cuda_stream), "begin")
                    L.check(l.vv_linear(C.byref(a), st.cuda_stream), "vv_linear")
                    ge = C.c_void_p()
                    L.check(l.vv_graph_end(st.cuda_stream, C.byref(ge)), "end")
                    L.check(l.vv_graph_launch(ge, st.cuda_stream), "launch")
                    st.synchronize()
                    l.vv_graph_destroy(ge)
                st.synchronize()
        finally:
            l.vv_tune(b"gemv_hot", -1)
        return self.buf.clone()

    def out_rows(self, image):
        o = self.at["out"]
        return image[o:o + self.m * self.ldo].view(self.m, self.ldo)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(6), ids=NAMES)
def test_hot_equals_template_on_carved_operands(lib, idx):
    c = _carved(lib, idx)
    e = c.e
    name = (C.c_char * 96)()
    lib.check(lib.load().vv_linear_route(C.byref(c.args()), name, 96), "route")
    assert name.value.decode() == f"gemv_hot<{idx}>"
    ref = c.run(0)
    rows = c.out_rows(ref)
    assert not torch.isnan(rows[:, :c.n]).any() and not torch.equal(rows[0, :c.n], rows[1, :c.n])
    # the template wrote the m x n outputs and nothing else; NaN == NaN under a bit compare of the images
    changed = ref.view(torch.int32) != c.image.view(torch.int32)
    assert int(changed.sum()) == c.m * c.n and bool(torch.isnan(rows[:, c.n:]).all())
    for graph in (False, True):
        got = c.run(1 << idx, graph=graph)
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), f"{e['name'].decode()} graph={graph}"


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(6), ids=NAMES)
def test_a_stride_beyond_31_bits_is_routed_to_the_template(lib, idx):
    """The entry's call with one of the strides its kernel takes as a 32-bit value set to 2^31 elements: described, never dereferenced."""
    c = _carved(lib, idx)
    e = c.e
    l = lib.load()
    fields = ["ldx"] + (["ld_mod"] if e["mod"] else []) + (["gate_ld"] if e["gate"] else []) + (["ldres"] if e["res"] else [])
    for f in fields:
        a = c.args()
        setattr(a, f, 1 << 31)
        name = (C.c_char * 96)()
        lib.check(l.vv_linear_route(C.byref(a), name, 96), "route")
        assert name.value.decode().startswith("gemv_stream<"), f"{e['name'].decode()} {f} = 2^31 -> {name.value.decode()}"
