"""The matrix-core GEMM on MXFP4 codes (csrc/vv_gemm_mx.hip, gemm_mx_kernel<dual, obf>) against an fp64 reference, per 32 x 32 output tile and
per row - through the C ABI only.

The kernel is reached through VV_LIN_W_MXGEMM with wdt == VV_MXFP4 alone.  Reference: plain fp64 on the effective weights quantize_mxfp4
returns (value(code) * 2^(e - 127), exact in bf16) and the bf16 activations as the device receives them, the epilogue in fp64, a bf16 output
rounded once (ref_linear_fp64 of tests/test_hip_mfma_gemm.py).  The device reads the same matrix as pack_mxfp4's companion.

Weights: the scale bytes of the k blocks walk 2^-20 .. 2^20 (BLOCK_EXP, the same exponent for a block column, times 2^(n % 3 - 1) per weight
row, plus whatever the block's own maximum adds) and the activations of a block column carry the inverse power of two, so every block's
products are O(1) and a block that is skipped, or decoded under its neighbour's scale, costs its row what the arithmetic says.  One block
(row 5, block 1) is all zero (scale byte 127), every e2m1 code occurs - the negative zero, code 8, is written over a few zero codes by hand,
quantize_mxfp4 never emits it.

Shapes: m in {3, 16, 17, 64, 130, 257} (fewer rows than a row tile; exactly one; one row in the second; a whole workgroup tile; two tiles and
two rows; four and one), n in {16, 48, 80, 272} (less than a wave's 64 channels; a ragged wave; a ragged workgroup tile; two tiles and a
quarter wave), k in {128, 512, 640, 1536, 2176} (one slab; one whole 512-unit; a ragged unit; three units; four and a ragged one) - all 120
with the plain epilogue, and every other epilogue on a walk through the same values that meets each of them.  Epilogues: plain, bias,
residual in its own array, residual in place, SwiGLU pair (fp32 out), SwiGLU pair with a bf16 output, plain with a bf16 output; ldx = k + 8,
ldo = ldres = n + 4, NaN in every gap and in two guard rows, two launches bit-identical, inputs bit-unchanged.

Bars: BAR["xb"] (1e-4) for fp32 outputs - that file's class for this arithmetic: bf16 activations, weights exact in bf16, fp32 sums - and
BAR["bf16"] (6e-3) where the output is rounded to bf16, both imported.  test_bars_sit_between_floor_and_dropped_block (CPU) holds every case to
that file's two conditions: bar >= FLOOR_HEADROOM x the error of an fp32 stand-in (32-wide k steps accumulated in fp32 in ascending order)
against the reference, and bar <= 1 / DROP_MARGIN of what one dropped 32-k block of one output row costs that row.
"""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from conftest import rel_rms
from test_hip_mfma_gemm import BAR, DROP_MARGIN, FLOOR_HEADROOM, Case, _FAKE, _epilogue, _lib, _need_gpu, _rel, _same_bits, built_kernels, fill_args, \
    instantiations_of, layout, ref_linear_fp64, route_of, tile_row_errors

LIN_W_MXGEMM = 32
VV_MXFP4, VV_MXFP4_FRAG = 4, 5
E_UNSUPPORTED = -3
BLOCK_EXP = (-20, 0, 20, -7, 5, 13, -13, 9, -3, 17, -17, 2)      # exponent of k block b: BLOCK_EXP[b % 12]


def _mx(dual, obf):
    return f"gemm_mx<dual={dual},obf={obf}>"


ALL_INSTANTIATIONS = [_mx(d, o) for d in (0, 1) for o in (0, 1)]
MS, NS, KS = (3, 16, 17, 64, 130, 257), (16, 48, 80, 272), (128, 512, 640, 1536, 2176)
EPILOGUES = {"plain": dict(), "bias": dict(bias=True), "res": dict(res="out"), "res_inplace": dict(res="inplace"), "swiglu": dict(act="swiglu"),
             "swiglu_bf16out": dict(act="swiglu", out_bf16=True), "bf16out": dict(out_bf16=True)}


def _cases():
    cs = []

    def add(m, n, k, name):
        kw = EPILOGUES[name]
        cs.append(Case(f"mx_m{m}_n{n}_k{k}_{name}", _mx(int(kw.get("act") == "swiglu"), int(bool(kw.get("out_bf16")))), m, n, k, **kw))

    for m in MS:
        for n in NS:
            for k in KS:
                add(m, n, k, "plain")
    for e, name in enumerate(list(EPILOGUES)[1:], 1):      # a walk that meets every m, and every n and k over the epilogues
        for i, m in enumerate(MS):
            add(m, NS[(i + e) % len(NS)], KS[(i + 2 * e) % len(KS)], name)
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


# ---------------------------------------------------------------------------------------------------------------
# operands: an MXFP4 matrix (codes, scale bytes, effective values) and activations scaled against its block exponents
# ---------------------------------------------------------------------------------------------------------------
def _block_exp(k):
    return torch.tensor([BLOCK_EXP[b % len(BLOCK_EXP)] for b in range(k // 32)], dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _weights(n, k, which):
    """(codes uint8 [n, k], scale bytes uint8 [n, k / 32], effective weights fp32 [n, k]) of matrix `which` (0: w, 1: w2)"""
    from vibevoice_rocm_amd.weights import quantize_mxfp4
    g = torch.Generator().manual_seed(zlib.crc32(repr(("mxw", n, k, which)).encode()))
    w = torch.randn(n, k, generator=g, dtype=torch.float64) / k ** 0.5
    w = w * torch.exp2(_block_exp(k)).repeat_interleave(32)[None, :] * torch.exp2((torch.arange(n) % 3 - 1).double())[:, None]
    if n > 5 and k >= 64:
        w[5, 32:64] = 0.0                                          # an all-zero block: scale byte 127
    codes, sb, eff = quantize_mxfp4(w.float().bfloat16())
    zeros = (codes == 0).nonzero()
    assert len(zeros) >= 3
    for r, c in zeros[:: max(1, len(zeros) // 3)][:3].tolist():     # the negative zero: the same effective value, another code
        codes[r, c] = 8
    assert set(codes.unique().tolist()) == set(range(16)), "every e2m1 code"
    assert int(sb.max()) - int(sb.min()) >= 40 and (n <= 5 or int(sb[5, 1]) == 127)
    return codes, sb, eff


@functools.lru_cache(maxsize=None)
def _x(k):
    """bf16 activations [257, k]: column block b carries 2^-BLOCK_EXP[b], so every block's products are O(1).  Calls of fewer rows take the
    first m: a row's operands do not depend on m"""
    g = torch.Generator().manual_seed(zlib.crc32(repr(("mxx", k)).encode()))
    x = torch.randn(max(MS), k, generator=g, dtype=torch.float64) * torch.exp2(-_block_exp(k)).repeat_interleave(32)[None, :]
    return x.float().bfloat16()


@functools.lru_cache(maxsize=None)
def _operands_of(key):
    m, n, k, bias, act, res = key
    g = torch.Generator().manual_seed(zlib.crc32(repr(("mxo", n, k)).encode()))
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
    from vibevoice_rocm_amd.weights import pack_mxfp4
    codes, sb, _ = _weights(n, k, which)
    return pack_mxfp4(codes, sb)


def mx_layout(case, o=None):
    """layout() of the bf16 case with the matrices replaced by their VV_MXFP4 companions: w / w2 = packed codes, wscale / w2scale = scale bytes"""
    buf, ld = layout(case, o or operands(case))
    buf["w"], buf["wscale"] = packed(case.n, case.k, 0)
    if case.dual:
        buf["w2"], buf["w2scale"] = packed(case.n, case.k, 1)
    return buf, ld


_FAKE_MX = dict(_FAKE, wscale=0x10000000 * 12, w2scale=0x10000000 * 13)


def mx_args(case, ld, ptr, flag=True):
    a = fill_args(case, ld, ptr)
    a.wdt, a.wscale = VV_MXFP4, ptr["wscale"]
    if case.dual:
        a.w2scale = ptr["w2scale"]
    if flag:
        a.flags |= LIN_W_MXGEMM
    return a


@functools.lru_cache(maxsize=None)
def _expect_of(key, out_bf16):
    """(fp64 reference, floor (global, tile, row) of the fp32 stand-in, cost to row 0 of one dropped 32-k block of that row)"""
    m, n, k, bias, act, res = key
    o = _operands_of(key)
    ref = ref_linear_fp64(o, "none", act, out_bf16, True)
    xh = o["x"].float()

    def steps(w):      # fp32 partial products of the 32-wide k steps
        return torch.bmm(xh.reshape(m, k // 32, 32).transpose(0, 1), w.float().reshape(n, k // 32, 32).permute(1, 2, 0))

    P, P2 = steps(o["w"]), steps(o["w2"]) if "w2" in o else None

    def acc(P, skip=None, rs=slice(None)):
        a = torch.zeros_like(P[0][rs])
        for s in range(P.shape[0]):
            if s != skip:
                a = a + P[s][rs]
        return a

    def finish(y, y2, rs=slice(None)):
        y = _epilogue(y, y2, o, act, torch.float32, rs)
        return (y.bfloat16() if out_bf16 else y).double()

    stand = finish(acc(P), acc(P2) if P2 is not None else None)
    t, _, r, _ = tile_row_errors(stand, ref)
    floor = (_rel(stand, ref), t, r)
    S, drop, r0 = k // 32, math.inf, slice(0, 1)
    for s0 in {0, S // 2, S - 1}:
        y = finish(acc(P, s0, r0), acc(P2, s0, r0) if P2 is not None else None, r0)
        drop = min(drop, _rel(y, ref[r0]))
    return ref, floor, drop


def expect(case):
    return _expect_of((case.m, case.n, case.k, case.bias, case.act, bool(case.res)), case.out_bf16)


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_flag_value_in_the_binding():
    L = _lib()[0]
    assert L.LIN_W_MXGEMM == LIN_W_MXGEMM and L.VV_MXFP4 == VV_MXFP4 and L.VV_MXFP4_FRAG == VV_MXFP4_FRAG


def test_every_instantiation_is_reached():
    """every instantiation has a case, every epilogue meets every row count, and every n and k is met by an epilogue other than the plain one"""
    assert {c.route for c in CASES} == set(ALL_INSTANTIATIONS)
    for name in EPILOGUES:
        assert {c.m for c in CASES if c.id.endswith("_" + name)} == set(MS), name
    rest = [c for c in CASES if not c.id.endswith("_plain")]
    assert {c.n for c in rest} == set(NS) and {c.k for c in rest} == set(KS)


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """vv_gemm_mx.hip's gfx950 code object holds the four instantiations of gemm_mx_kernel and no other (CPU only: symbol names of the object
    file build() left)"""
    got = instantiations_of(built_kernels("vv_gemm_mx.hip", tmp_path), {"gemm_mx_kernel": _mx})
    assert got == set(ALL_INSTANTIATIONS), sorted(got ^ set(ALL_INSTANTIATIONS))


@pytest.mark.parametrize("cid", CASE_IDS)
def test_route_of_every_case_on_the_host(cid):
    """stand-in addresses, nothing launched: the route query names the instantiation the case is meant for"""
    case = CASES[CASE_IDS.index(cid)]
    assert route_of(mx_args(case, layout(case, operands(case))[1], _FAKE_MX)) == case.route


def _route_rc(a):
    L, l = _lib()[:2]
    name = C.create_string_buffer(96)
    return l.vv_linear_route(C.byref(a), name, 96), name.value.decode(), l.vv_last_error().decode()


def test_refusals_on_the_host():
    """Every refusal of the new flag is VV_E_UNSUPPORTED from the route query (the checks vv_linear runs before it launches), and the calls
    that were refused without the flag still are."""
    L = _lib()[0]
    ok = Case("r_ok", "", 9, 48, 640, bias=True, res="out")
    ld = layout(ok, operands(ok))[1]
    assert _route_rc(mx_args(ok, ld, _FAKE_MX))[:2] == (0, _mx(0, 0))

    def refused(a, what):
        rc, name, err = _route_rc(a)
        assert rc == E_UNSUPPORTED and name == "", (what, rc, name, err)

    a = mx_args(ok, ld, _FAKE_MX)
    a.flags &= ~L.LIN_X_BF16
    refused(a, "the bit without VV_LIN_X_BF16")
    for what, case in (("n % 16", Case("r_n", "", 9, 40, 640)), ("k % 128", Case("r_k", "", 9, 48, 576)), ("m < 3", Case("r_m", "", 2, 48, 640))):
        refused(mx_args(case, layout(case, _like(case))[1], _FAKE_MX), what)
    a = mx_args(ok, ld, _FAKE_MX)
    a.wscale = None
    refused(a, "missing scales")
    dual = Case("r_dual", "", 9, 48, 640, act="swiglu")
    a = mx_args(dual, layout(dual, operands(dual))[1], _FAKE_MX)
    a.w2scale = None
    refused(a, "missing w2 scales")
    a = mx_args(ok, ld, _FAKE_MX)
    a.pro, a.norm_w = L.PRO_RMSNORM, _FAKE_MX["norm_w"]
    refused(a, "a prologue")
    a = mx_args(ok, ld, _FAKE_MX)
    a.wdt = L.VV_BF16
    refused(a, "the bit on bf16 weights")
    a = mx_args(ok, ld, dict(_FAKE_MX, w=_FAKE_MX["w"] + 8))
    refused(a, "misaligned codes")
    # refused before this flag existed, refused now: VV_MXFP4 at 9 rows without the bit (fp32 x, as such a call would come), and
    # VV_MXFP4_FRAG with a bf16 x
    a = mx_args(Case("r_9", "", 9, 48, 640, xb=False), ld, _FAKE_MX, flag=False)
    refused(a, "VV_MXFP4 at m = 9 without the bit")
    a = mx_args(Case("r_9b", "", 9, 48, 640), ld, _FAKE_MX, flag=False)
    refused(a, "VV_MXFP4 at m = 9 with a bf16 x, without the bit")
    a = mx_args(Case("r_frag", "", 4, 48, 640), ld, _FAKE_MX, flag=False)
    a.wdt, a.flags = VV_MXFP4_FRAG, a.flags | L.LIN_W_FRAG
    refused(a, "VV_MXFP4_FRAG with VV_LIN_X_BF16")


def _like(case):
    """operands for the layout of a refused shape (strides only: no MXFP4 matrix of that shape need exist)"""
    return {"x": torch.zeros(case.m, case.k, dtype=torch.bfloat16), "w": torch.zeros(case.n, case.k, dtype=torch.bfloat16)}


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
def _run(case, o=None):
    """two launches into separate outputs, bit-identical; NaN gaps and guards intact; inputs unchanged.  Returns the raw [m, n] output"""
    L, l = _lib()[:2]
    buf, ld = mx_layout(case, o)
    m, n, ldo = case.m, case.n, ld["ldo"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda(), buf["out"].cuda()]
    for out in outs:
        a = mx_args(case, ld, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
        assert route_of(a) == case.route, (case.id, route_of(a))
        L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    h0, h1 = outs[0].cpu(), outs[1].cpu()
    assert _same_bits(h0, h1), f"{case.id}: two runs of the same call differ"
    for name, t in dev.items():
        assert _same_bits(t.cpu(), buf[name]), f"{case.id}: input {name} was written"
    grid = h0.view(m + 2, ldo)
    inside = torch.zeros(m + 2, ldo, dtype=torch.bool)
    inside[:m, :n] = True
    assert torch.isfinite(grid[inside]).all(), f"{case.id}: {int((~torch.isfinite(grid[inside])).sum())} in-range outputs are not finite"
    assert torch.isnan(grid[~inside]).all(), f"{case.id}: a gap or guard element of out was written"
    return grid[:m, :n].contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gemm_mx_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    ref = expect(case)[0].numpy()
    got = _run(case).double().numpy()
    g = rel_rms(got, ref, f"{cid} [{case.route}] global")
    t, ti, r, ri = tile_row_errors(got, ref)
    # the worst single element, against |its reference value| + the output's rms: an fp32 sum errs by ~ sqrt(K) 2^-24 of the rms (3e-6 at the
    # longest K), a bf16 output by at most one ulp (2^-8 = 3.9e-3) of its own value; a dropped 32-k block moves an element by ~ sqrt(32 / K) of
    # the rms (>= 0.12 here).  The class bar sits between, so it holds for this figure as it does for the tile and the row
    worst = float(np.max(np.abs(got - ref) / (np.abs(ref) + np.sqrt(np.mean(ref ** 2)) + 1e-300)))
    bar = BAR[case.klass]
    print(f"{cid}: {case.route} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst tile {t:.3e} at (row tile {ti[0]}, channel tile {ti[1]})  "
          f"worst row {r:.3e} (row {ri})  worst element {worst:.3e}")
    assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
    assert t < bar, f"{cid}: 32 x 32 tile (row tile {ti[0]}, channel tile {ti[1]}) rel RMS {t:.3e} >= {bar:.1e}"
    assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"
    assert worst < bar, f"{cid}: worst element error {worst:.3e} of (|ref| + rms) >= {bar:.1e}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bias", "res", "swiglu_bf16out"])
def test_permuted_rows_give_permuted_rows_bit_for_bit(name):
    _need_gpu()
    kw = EPILOGUES[name]
    case = Case(f"perm_{name}", _mx(int(kw.get("act") == "swiglu"), int(bool(kw.get("out_bf16")))), 130, 80, 640, **kw)
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
    route = _mx(int(kw.get("act") == "swiglu"), int(bool(kw.get("out_bf16"))))
    for n, k in ((80, 640), (272, 2176)):
        big, small = Case(f"big_{name}", route, 130, n, k, **kw), Case(f"small_{name}", route, 3, n, k, **kw)
        assert _same_bits(_run(big)[:3].contiguous(), _run(small)), (name, n, k)


@pytest.mark.gpu
def test_refused_calls_launch_nothing():
    """vv_linear itself: VV_E_UNSUPPORTED and an untouched output for a refusal of the new flag"""
    _need_gpu()
    L, l = _lib()[:2]
    case = Case("rg", "", 9, 48, 640)
    buf, ld = mx_layout(case)
    dev = {name: t.cuda() for name, t in buf.items()}
    a = mx_args(case, ld, {name: t.data_ptr() for name, t in dev.items()})
    a.k = 576
    assert l.vv_linear(C.byref(a), None) == E_UNSUPPORTED
    a = mx_args(case, ld, {name: t.data_ptr() for name, t in dev.items()})
    a.flags &= ~L.LIN_X_BF16
    assert l.vv_linear(C.byref(a), None) == E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(dev["out"].cpu()).all()
