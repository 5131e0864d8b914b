"""The matrix-core GEMM on MXFP6 (e2m3) codes (csrc/vv_gemm_mx6.hip, gemm_mx6_kernel<dual, obf>) against an fp64 reference, per 32 x 32 output
tile and per row - through the C ABI only.  The MXFP6 image of tests/test_hip_gemm_mx.py.

The kernel is reached through VV_LIN_W_MX6GEMM (64) with wdt == VV_MXFP6 alone; VV_MXFP6 with VV_LIN_W_MXGEMM (32) stays refused.  Reference:
plain fp64 on the effective weights quantize_mxfp6 returns (value(code) * 2^(e - 127), exact in bf16) and the bf16 activations as the device
receives them, the epilogue in fp64, a bf16 output rounded once (ref_linear_fp64 of tests/test_hip_mfma_gemm.py).  The device reads the same
matrix as pack_mxfp6's companion (two planes per row group, scale dwords beside them).

Weights: the scale bytes of the k blocks walk 2^-20 .. 2^20 (BLOCK_EXP, the same exponent for a block column, times 2^(n % 3 - 1) per weight
row, plus whatever the block's own maximum adds) and the activations of a block column carry the inverse power of two, so every block's
products are O(1) and a block that is skipped, or decoded under its neighbour's scale, costs its row what the arithmetic says.  One block
(row 5, block 1) is all zero (scale byte 127), every one of the 64 e2m3 codes occurs - the negative zero, code 32, is written over a few zero
codes by hand, quantize_mxfp6 never emits it.

Shapes: m in {3, 16, 17, 64, 130} (fewer rows than a row tile; exactly one; one row in the second; a whole workgroup tile; two tiles and two
rows), n in {16, 48, 80, 272} against a wave's 32 channels and a workgroup tile of 64 (half a wave; a ragged wave and a ragged tile; a tile and
half a wave; four tiles and half a wave), k in {128, 256, 384, 640} (one slab; an even and an odd number of slabs across the two LDS buffers;
five slabs) - all 80 with the plain epilogue, and every other epilogue on a walk through the same values that meets each of them.  Epilogues:
plain, bias, residual in its own array, residual in place, SwiGLU pair (fp32 out), SwiGLU pair with a bf16 output, plain with a bf16 output;
ldx = k + 8, ldo = ldres = n + 4, NaN in every gap and in two guard rows, two launches bit-identical, inputs bit-unchanged.

Bars: BAR["xb"] (1e-4) for fp32 outputs - that file's class for this arithmetic: bf16 activations, weights exact in bf16, fp32 sums - and
BAR["bf16"] (6e-3) where the output is rounded to bf16, both imported.  test_bars_sit_between_floor_and_dropped_block (CPU) holds every case to
that file's two conditions: bar >= FLOOR_HEADROOM x the error of an fp32 stand-in that sums in the kernel's k order (the 128-wide steps
ascending, inside a step h = 0..3, MFMA h holding k = 128 J + 32 c + 8 h + i) against the reference, and bar <= 1 / DROP_MARGIN of what one
dropped 32-k block of one output row costs that row.
"""
import ctypes as C
import functools
import math
import os
import re
import zlib

import numpy as np
import pytest
import torch

from conftest import rel_rms
from test_hip_mfma_gemm import BAR, DROP_MARGIN, FLOOR_HEADROOM, Case, _FAKE, _epilogue, _lib, _need_gpu, _rel, _same_bits, built_kernels, fill_args, \
    instantiations_of, layout, ref_linear_fp64, route_of, tile_row_errors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIN_W_MXGEMM, LIN_W_MX6GEMM = 32, 64
VV_MXFP4, VV_MXFP6, VV_MXFP6_FRAG = 4, 6, 8
E_UNSUPPORTED = -3
BLOCK_EXP = (-20, 0, 20, -7, 5, 13, -13, 9, -3, 17, -17, 2)      # exponent of k block b: BLOCK_EXP[b % 12]


def _mx6(dual, obf):
    return f"gemm_mx6<dual={dual},obf={obf}>"


def _mx4(dual, obf):
    return f"gemm_mx<dual={dual},obf={obf}>"


ALL_INSTANTIATIONS = [_mx6(d, o) for d in (0, 1) for o in (0, 1)]
MS, NS, KS = (3, 16, 17, 64, 130), (16, 48, 80, 272), (128, 256, 384, 640)
EPILOGUES = {"plain": dict(), "bias": dict(bias=True), "res": dict(res="out"), "res_inplace": dict(res="inplace"), "swiglu": dict(act="swiglu"),
             "swiglu_bf16out": dict(act="swiglu", out_bf16=True), "bf16out": dict(out_bf16=True)}


def _cases():
    cs = []

    def add(m, n, k, name):
        kw = EPILOGUES[name]
        cs.append(Case(f"mx6_m{m}_n{n}_k{k}_{name}", _mx6(int(kw.get("act") == "swiglu"), int(bool(kw.get("out_bf16")))), m, n, k, **kw))

    for m in MS:
        for n in NS:
            for k in KS:
                add(m, n, k, "plain")
    for e, name in enumerate(list(EPILOGUES)[1:], 1):      # a walk that meets every m, and every n and k over the epilogues
        for i, m in enumerate(MS):
            add(m, NS[(i + e) % len(NS)], KS[(i + 2 * e + e // 4) % len(KS)], name)
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


# ---------------------------------------------------------------------------------------------------------------
# operands: an MXFP6 matrix (codes, scale bytes, effective values) and activations scaled against its block exponents
# ---------------------------------------------------------------------------------------------------------------
def _block_exp(k):
    return torch.tensor([BLOCK_EXP[b % len(BLOCK_EXP)] for b in range(k // 32)], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _weights(n, k, which):
    """(codes uint8 [n, k], scale bytes uint8 [n, k / 32], effective weights fp32 [n, k]) of matrix `which` (0: w, 1: w2)"""
    from vibevoice_rocm_amd.weights import quantize_mxfp6
    g = torch.Generator().manual_seed(zlib.crc32(repr(("mx6w", n, k, which)).encode()))
    w = torch.randn(n, k, generator=g, dtype=torch.float64) / k ** 0.5
    w = w * torch.exp2(_block_exp(k)).repeat_interleave(32)[None, :] * torch.exp2((torch.arange(n) % 3 - 1).double())[:, None]
    if n > 5 and k >= 64:
        w[5, 32:64] = 0.0                                          # an all-zero block: scale byte 127
    codes, sb, eff = quantize_mxfp6(w.float().bfloat16())
    zeros = (codes == 0).nonzero()
    assert len(zeros) >= 3
    for r, c in zeros[:: max(1, len(zeros) // 3)][:3].tolist():     # the negative zero: the same effective value, another code
        codes[r, c] = 32
    assert set(codes.unique().tolist()) == set(range(64)), "every e2m3 code"
    assert int(sb.max()) - int(sb.min()) >= 40 and (n <= 5 or k < 64 or int(sb[5, 1]) == 127)
    return codes, sb, eff


@functools.lru_cache(maxsize=None)
def _x(k):
    """bf16 activations [130, k]: column block b carries 2^-BLOCK_EXP[b], so every block's products are O(1).  Calls of fewer rows take the
    first m: a row's operands do not depend on m"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(("mx6x", k)).encode()))
    x = torch.randn(max(MS), k, generator=g, dtype=torch.float64) * torch.exp2(-_block_exp(k)).repeat_interleave(32)[None, :]
    return x.float().bfloat16()


@functools.lru_cache(maxsize=None)
def _operands_of(key):
    m, n, k, bias, act, res = key
    g = torch.Generator().manual_seed(zlib.crc32(repr(("mx6o", n, k)).encode()))
    o = {"x": _x(k)[:m].contiguous(), "w": _weights(n, k, 0)[2].bfloat16()}
    assert torch.equal(o["w"].float(), _weights(n, k, 0)[2]), "the effective weights are exact in bf16"
    if act == "swiglu":
        o["w2"] = _weights(n, k, 1)[2].bfloat16()
    b, r = 0.1 * torch.randn(n, generator=g), torch.randn(max(MS), n, generator=g)
    if bias:
        o["bias"] = b
    if res:
        o["res"] = r[:m].contiguous()
    return o


def operands(case):
    return _operands_of((case.m, case.n, case.k, case.bias, case.act, bool(case.res)))


def packed(n, k, which):
    from vibevoice_rocm_amd.weights import pack_mxfp6
    codes, sb, _ = _weights(n, k, which)
    return pack_mxfp6(codes, sb)


def mx_layout(case, o=None):
    """layout() of the bf16 case with the matrices replaced by their VV_MXFP6 companions: w / w2 = packed codes, wscale / w2scale = scale bytes"""
    buf, ld = layout(case, o or operands(case))
    buf["w"], buf["wscale"] = packed(case.n, case.k, 0)
    if case.dual:
        buf["w2"], buf["w2scale"] = packed(case.n, case.k, 1)
    return buf, ld


_FAKE_MX = dict(_FAKE, wscale=0x10000000 * 12, w2scale=0x10000000 * 13)


def mx_args(case, ld, ptr, flag=LIN_W_MX6GEMM):
    a = fill_args(case, ld, ptr)
    a.wdt, a.wscale = VV_MXFP6, ptr["wscale"]
    if case.dual:
        a.w2scale = ptr["w2scale"]
    a.flags |= flag
    return a


def _kernel_order(t, k):
    """[.., k] -> [.., k / 32, 32]: the 32-wide groups the kernel's MFMAs sum, in the order an accumulator meets them - 128-wide step J
    ascending, inside it h = 0..3, MFMA h holding k = 128 J + 32 c + 8 h + i (c = 0..3, i = 0..7)"""
    lead = t.shape[:-1]
    return t.reshape(*lead, k // 128, 4, 4, 8).transpose(-3, -2).reshape(*lead, k // 32, 32)


@functools.lru_cache(maxsize=None)
def _expect_of(key, out_bf16):
    """(fp64 reference, floor (global, tile, row) of the fp32 stand-in, cost to row 0 of one dropped 32-k block of that row)"""
    m, n, k, bias, act, res = key
    o = _operands_of(key)
    ref = ref_linear_fp64(o, "none", act, out_bf16, True)
    xh = o["x"].float()

    def steps(w, x=xh, drop=None):      # fp32 partial products of the kernel's 32-wide MFMA groups; drop: MX block (k = 32 b .. + 31) left out
        w = w.float().clone()
        if drop is not None:
            w[:, 32 * drop: 32 * drop + 32] = 0.0
        return torch.bmm(_kernel_order(x, k).transpose(0, 1), _kernel_order(w, k).permute(1, 2, 0))

    def acc(P):
        a = torch.zeros_like(P[0])
        for s in range(P.shape[0]):
            a = a + P[s]
        return a

    def finish(y, y2, rs=slice(None)):
        y = _epilogue(y, y2, o, act, torch.float32, rs)
        return (y.bfloat16() if out_bf16 else y).double()

    stand = finish(acc(steps(o["w"])), acc(steps(o["w2"])) if "w2" in o else None)
    t, _, r, _ = tile_row_errors(stand, ref)
    floor = (_rel(stand, ref), t, r)
    S, drop, r0 = k // 32, math.inf, slice(0, 1)
    for s0 in {0, S // 2, S - 1}:
        y = finish(acc(steps(o["w"], xh[r0], s0)), acc(steps(o["w2"], xh[r0], s0)) if "w2" in o else None, r0)
        drop = min(drop, _rel(y, ref[r0]))
    return ref, floor, drop


def expect(case):
    return _expect_of((case.m, case.n, case.k, case.bias, case.act, bool(case.res)), case.out_bf16)


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_flag_value_in_the_header_and_the_binding():
    L = _lib()[0]
    assert L.LIN_W_MX6GEMM == LIN_W_MX6GEMM and L.LIN_W_MXGEMM == LIN_W_MXGEMM and L.VV_MXFP6 == VV_MXFP6 and L.VV_MXFP6_FRAG == VV_MXFP6_FRAG
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    assert re.search(r"^enum \{ VV_LIN_W_MX6GEMM = 64 \};$", hdr, re.M), "an enum line of its own"
    assert re.search(r"VV_LIN_PACKED = 16, VV_LIN_W_MXGEMM = 32 \};", hdr), "the existing flags line is as it was"
    assert L.load().vv_abi_version() == 6


def test_every_instantiation_is_reached():
    """every instantiation has a case, every epilogue meets every row count, and every n and k is met by an epilogue other than the plain one"""
    assert {c.route for c in CASES} == set(ALL_INSTANTIATIONS)
    for name in EPILOGUES:
        assert {c.m for c in CASES if c.id.endswith("_" + name)} == set(MS), name
    rest = [c for c in CASES if not c.id.endswith("_plain")]
    assert {c.n for c in rest} == set(NS) and {c.k for c in rest} == set(KS)
    assert {(c.m, c.n, c.k) for c in CASES if c.id.endswith("_plain")} == {(m, n, k) for m in MS for n in NS for k in KS}


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """vv_gemm_mx6.hip's gfx950 code object holds the four instantiations of gemm_mx6_kernel and no other kernel, vv_gemm_mx.hip's still its four
    (CPU only: symbol names of the object files build() left), and the unit is part of the build"""
    from vibevoice_rocm_amd import build
    assert any(s.endswith("vv_gemm_mx6.hip") for s in build.SRC)
    kernels = built_kernels("vv_gemm_mx6.hip", tmp_path, plain=True)
    assert {k for k, _ in kernels} == {"gemm_mx6_kernel"}, kernels
    got = instantiations_of(kernels, {"gemm_mx6_kernel": _mx6})
    assert got == set(ALL_INSTANTIATIONS), sorted(got ^ set(ALL_INSTANTIATIONS))
    got4 = instantiations_of(built_kernels("vv_gemm_mx.hip", tmp_path), {"gemm_mx_kernel": _mx4})
    assert got4 == {_mx4(d, o) for d in (0, 1) for o in (0, 1)}, sorted(got4)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_route_of_every_case_on_the_host(cid):
    """stand-in addresses, nothing launched: the route query names the instantiation the case is meant for"""
    case = CASES[CASE_IDS.index(cid)]
    assert route_of(mx_args(case, layout(case, operands(case))[1], _FAKE_MX)) == case.route


def _route_rc(a):
    L, l = _lib()[:2]
    name = C.create_string_buffer(96)
    return l.vv_linear_route(C.byref(a), name, 96), name.value.decode(), l.vv_last_error().decode()


def _like(case):
    """operands for the layout of a shape (strides only: no MXFP6 matrix of that shape need exist)"""
    o = {"x": torch.zeros(case.m, case.k, dtype=torch.bfloat16), "w": torch.zeros(case.n, case.k, dtype=torch.bfloat16)}
    if case.dual:
        o["w2"] = o["w"]
    if case.bias:
        o["bias"] = torch.zeros(case.n)
    if case.res:
        o["res"] = torch.zeros(case.m, case.n)
    return o


def _set(**kw):
    def f(a, L):
        for name, v in kw.items():
            setattr(a, name, v)
    return f


def _bump(field, by):
    def f(a, L):
        setattr(a, field, getattr(a, field) + by)
    return f


def _faults(L):
    """(what, the case the call is built from, what is done to the routed call): every refusal the issue's routing rules list"""
    ok, dual = Case("r_ok", "", 9, 48, 640, bias=True, res="out"), Case("r_dual", "", 9, 48, 640, act="swiglu")
    F = [("wdt VV_MXFP4", ok, _set(wdt=VV_MXFP4)), ("wdt VV_BF16", ok, _set(wdt=L.VV_BF16)), ("wdt VV_MXFP6_FRAG", ok, _set(wdt=VV_MXFP6_FRAG)),
         ("wdt VV_FP8", ok, _set(wdt=L.VV_FP8)), ("wdt VV_F32", ok, _set(wdt=L.VV_F32)),
         ("both GEMM bits", ok, lambda a, L: setattr(a, "flags", a.flags | LIN_W_MXGEMM)),
         ("VV_LIN_W_FRAG", ok, lambda a, L: setattr(a, "flags", a.flags | L.LIN_W_FRAG)),
         ("fp32 x", ok, lambda a, L: setattr(a, "flags", a.flags & ~L.LIN_X_BF16)),
         ("an RMSNorm prologue", ok, _set(pro=L.PRO_RMSNORM, norm_w=_FAKE_MX["norm_w"])), ("a SiLU prologue", ok, _set(pro=L.PRO_SILU)),
         ("m < 3", ok, _set(m=2)), ("n % 16", ok, _set(n=40)), ("k % 128", ok, _set(k=576)), ("k % 128 (a whole MX block more)", ok, _set(k=672)),
         ("missing scales", ok, _set(wscale=None)), ("missing w2 scales", dual, _set(w2scale=None)),
         ("a channel gate", ok, _set(gate=_FAKE_MX["gate"])), ("a row gate", ok, _set(gate=_FAKE_MX["gate"], gate_ld=52)),
         ("GELU", ok, _set(act=L.ACT_GELU)),
         ("misaligned codes", ok, _bump("w", 8)), ("misaligned w2 codes", dual, _bump("w2", 8)), ("misaligned scale bytes", ok, _bump("wscale", 2)),
         ("misaligned w2 scale bytes", dual, _bump("w2scale", 2)), ("misaligned x", ok, _bump("x", 8)), ("ldx % 8", ok, _bump("ldx", 4)),
         ("misaligned out", ok, _bump("out", 8)), ("ldo % 4", ok, _bump("ldo", 2)), ("misaligned bias", ok, _bump("bias", 4)),
         ("misaligned res", ok, _bump("res", 8)), ("ldres % 4", ok, _bump("ldres", 1))]
    return F


def test_refusals_on_the_host():
    """Every refusal of the new flag is VV_E_UNSUPPORTED with an empty name from the route query (the checks vv_linear runs before it launches);
    the same call without the fault is routed; and the calls that were refused before the flag existed still are."""
    L = _lib()[0]
    for what, case, fault in _faults(L):
        a = mx_args(case, layout(case, _like(case))[1], _FAKE_MX)
        assert _route_rc(a)[:2] == (0, _mx6(int(case.dual), 0)), what      # the call with the fault repaired
        fault(a, L)
        rc, name, err = _route_rc(a)
        assert rc == E_UNSUPPORTED and name == "", (what, rc, name, err)
    # scale bytes need 4-byte alignment only (codes 16): a scale address 4 past a 16-byte boundary is taken
    ok = Case("r_ok", "", 9, 48, 640)
    a = mx_args(ok, layout(ok, _like(ok))[1], _FAKE_MX)
    a.wscale += 4
    assert _route_rc(a)[:2] == (0, _mx6(0, 0))
    # pinned refused before this flag existed, refused now: VV_MXFP6 with VV_LIN_W_MXGEMM | VV_LIN_X_BF16 (tests/test_hip_mxfp6.py,
    # tests/test_host_rowbatch_mxfp6.py), with or without a bf16 output; VV_MXFP6 at 9 rows without any bit; VV_MXFP6_FRAG with the new bit
    for case in (ok, Case("r_obf", "", 9, 48, 640, out_bf16=True)):
        rc, name, err = _route_rc(mx_args(case, layout(case, _like(case))[1], _FAKE_MX, flag=LIN_W_MXGEMM))
        assert rc == E_UNSUPPORTED and name == "", ("VV_MXFP6 with VV_LIN_W_MXGEMM", rc, name, err)
    for xb in (False, True):
        case = Case("r_9", "", 9, 48, 640, xb=xb)
        rc, name, err = _route_rc(mx_args(case, layout(case, _like(case))[1], _FAKE_MX, flag=0))
        assert rc == E_UNSUPPORTED and name == "", ("VV_MXFP6 at m = 9 without the bit", xb, rc, name, err)
    case = Case("r_frag", "", 4, 48, 640, xb=False)
    a = mx_args(case, layout(case, _like(case))[1], _FAKE_MX)
    a.wdt, a.flags = VV_MXFP6_FRAG, a.flags | L.LIN_W_FRAG
    rc, name, err = _route_rc(a)
    assert rc == E_UNSUPPORTED and name == "", ("VV_MXFP6_FRAG with the bit", rc, name, err)
    # the MXFP4 GEMM's own calls are decided as before
    a = mx_args(ok, layout(ok, _like(ok))[1], _FAKE_MX, flag=LIN_W_MXGEMM)
    a.wdt = VV_MXFP4
    a.wscale = _FAKE_MX["wscale"]
    assert _route_rc(a)[:2] == (0, _mx4(0, 0))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_bars_sit_between_floor_and_dropped_block(cid):
    case = CASES[CASE_IDS.index(cid)]
    _, floor, drop = expect(case)
    bar = BAR[case.klass]
    print(f"{cid}: class {case.klass} bar {bar:.1e}  floor global {floor[0]:.2e} tile {floor[1]:.2e} row {floor[2]:.2e}  dropped block {drop:.2e}")
    assert bar >= FLOOR_HEADROOM * max(floor), (cid, bar, floor)
    assert bar <= drop / DROP_MARGIN, (cid, bar, drop)


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def _launch(case, buf, ld, runs=2):
    """`runs` launches into separate outputs, bit-identical; NaN gaps and guards intact; inputs unchanged.  Returns the raw [m, n] output"""
    L, l = _lib()[:2]
    m, n, ldo = case.m, case.n, ld["ldo"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda() for _ in range(runs)]
    for out in outs:
        a = mx_args(case, ld, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
        assert route_of(a) == case.route, (case.id, route_of(a))
        L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    hs = [o.cpu() for o in outs]
    for h in hs[1:]:
        assert _same_bits(hs[0], h), f"{case.id}: two runs of the same call differ"
    for name, t in dev.items():
        assert _same_bits(t.cpu(), buf[name]), f"{case.id}: input {name} was written"
    grid = hs[0].view(m + 2, ldo)
    inside = torch.zeros(m + 2, ldo, dtype=torch.bool)
    inside[:m, :n] = True
    assert torch.isfinite(grid[inside]).all(), f"{case.id}: {int((~torch.isfinite(grid[inside])).sum())} in-range outputs are not finite"
    assert torch.isnan(grid[~inside]).all(), f"{case.id}: a gap or guard element of out was written"
    return grid[:m, :n].contiguous()


def _run(case, o=None):
    return _launch(case, *mx_layout(case, o))


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gemm_mx6_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    ref = expect(case)[0].numpy()
    got = _run(case).double().numpy()
    g = rel_rms(got, ref, f"{cid} [{case.route}] global")
    t, ti, r, ri = tile_row_errors(got, ref)
    # the worst single element, against |its reference value| + the output's rms: an fp32 sum errs by ~ sqrt(K) 2^-24 of the rms (2e-6 at the
    # longest K), a bf16 output by at most one ulp (2^-8 = 3.9e-3) of its own value; a dropped 32-k block moves an element by ~ sqrt(32 / K) of
    # the rms (>= 0.22 here).  The class bar sits between, so it holds for this figure as it does for the tile and the row
    worst = float(np.max(np.abs(got - ref) / (np.abs(ref) + np.sqrt(np.mean(ref ** 2)) + 1e-300)))
    bar = BAR[case.klass]
    print(f"{cid}: {case.route} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst tile {t:.3e} at (row tile {ti[0]}, channel tile {ti[1]})  "
          f"worst row {r:.3e} (row {ri})  worst element {worst:.3e}")
    assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
    assert t < bar, f"{cid}: 32 x 32 tile (row tile {ti[0]}, channel tile {ti[1]}) rel RMS {t:.3e} >= {bar:.1e}"
    assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"
    assert worst < bar, f"{cid}: worst element error {worst:.3e} of (|ref| + rms) >= {bar:.1e}"


@pytest.mark.gpu
@pytest.mark.parametrize("e", [2, 127, 252])
def test_decode_is_exact(e):
    """One-hot bf16 activations read the matrix back: out[j, n] = W_eff[n, j], exactly.  codes[n, j] = (n + j) % 64 over 64 rows x 256 k puts every
    code at every position of a block (and in both LDS buffers); one scale byte for all blocks: 2 (the smallest elements are fp32 subnormals, down
    to 2^-128), 127 and 252 (7.5 x 2^125).  The matrix-core product and the conversion deliver every one of them un-flushed and un-rounded."""
    _need_gpu()
    from vibevoice_rocm_amd.weights import MXFP6_VALUES, pack_mxfp6
    n, k = 64, 256
    case = Case(f"exact_e{e}", _mx6(0, 0), k, n, k)
    codes = ((torch.arange(n)[:, None] + torch.arange(k)[None, :]) % 64).to(torch.uint8)
    for p in range(32):
        assert set(codes[:, p::32].unique().tolist()) == set(range(64))
    sb = torch.full((n, k // 32), e, dtype=torch.uint8)
    mag = torch.tensor(MXFP6_VALUES, dtype=torch.float64)[(codes & 31).long()]
    eff = (torch.where(codes >= 32, -mag, mag) * 2.0 ** (e - 127)).float()
    assert torch.equal(eff.double(), torch.where(codes >= 32, -mag, mag) * 2.0 ** (e - 127)) and torch.isfinite(eff).all()
    assert e != 2 or float(eff.abs()[eff != 0].min()) == 2.0 ** -128
    buf, ld = layout(case, {"x": torch.eye(k, dtype=torch.bfloat16), "w": eff.bfloat16()})
    buf["w"], buf["wscale"] = pack_mxfp6(codes, sb)
    got = _launch(case, buf, ld)
    bad = (got != eff.t()).nonzero()
    print(f"scale byte {e}: {len(bad)} of {n * k} weights read back wrong; smallest non-zero magnitude {float(eff.abs()[eff != 0].min()):.3e}")
    assert len(bad) == 0, (e, bad[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bias", "res", "swiglu_bf16out"])
def test_permuted_rows_give_permuted_rows_bit_for_bit(name):
    _need_gpu()
    kw = EPILOGUES[name]
    case = Case(f"perm_{name}", _mx6(int(kw.get("act") == "swiglu"), int(bool(kw.get("out_bf16")))), 130, 80, 640, **kw)
    o = dict(operands(case))
    base = _run(case, o)
    perm = torch.randperm(case.m, generator=torch.Generator().manual_seed(5))
    o["x"] = o["x"][perm].contiguous()
    if "res" in o:
        o["res"] = o["res"][perm].contiguous()
    assert _same_bits(_run(case, o), base[perm].contiguous())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bias", "res_inplace", "swiglu", "swiglu_bf16out"])
def test_first_rows_of_a_large_call_equal_the_small_call_bit_for_bit(name):
    """rows 0..2 of the m = 130 call are the m = 3 call on those rows: the result of a row does not depend on which rows share the call"""
    _need_gpu()
    kw = EPILOGUES[name]
    route = _mx6(int(kw.get("act") == "swiglu"), int(bool(kw.get("out_bf16"))))
    for n, k in ((80, 640), (272, 384)):
        big, small = Case(f"big_{name}", route, 130, n, k, **kw), Case(f"small_{name}", route, 3, n, k, **kw)
        assert _same_bits(_run(big)[:3].contiguous(), _run(small)), (name, n, k)


@pytest.mark.gpu
def test_refused_calls_launch_nothing():
    """vv_linear itself: VV_E_UNSUPPORTED and an untouched output for every refusal of the new flag, and for the pinned VV_LIN_W_MXGEMM call"""
    _need_gpu()
    L, l = _lib()[:2]
    outs = []
    for what, case, fault in _faults(L):
        buf, ld = mx_layout(case)
        dev = {name: t.cuda() for name, t in buf.items()}
        a = mx_args(case, ld, {name: t.data_ptr() for name, t in dev.items()})
        fault(a, L)
        assert l.vv_linear(C.byref(a), None) == E_UNSUPPORTED, what
        outs.append((what, dev))
    case = Case("rg", "", 9, 48, 640)
    buf, ld = mx_layout(case)
    dev = {name: t.cuda() for name, t in buf.items()}
    a = mx_args(case, ld, {name: t.data_ptr() for name, t in dev.items()}, flag=LIN_W_MXGEMM)
    assert l.vv_linear(C.byref(a), None) == E_UNSUPPORTED
    outs.append(("VV_MXFP6 with VV_LIN_W_MXGEMM", dev))
    torch.cuda.synchronize()
    for what, dev in outs:
        assert _same_bits(dev["out"].cpu(), buf_nan(dev["out"])), what


def buf_nan(t):
    return torch.full(t.shape, float("nan"), dtype=t.dtype)
