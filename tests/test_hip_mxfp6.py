"""Weight-only OCP MXFP6 e2m3 (weight_quant="mxfp6", vv_linear's VV_MXFP6 form: gemv_mx6_kernel, csrc/vv_gemv_mx6.hip) on the MI355X.

1. `test_decode_is_exact`: one matrix with all 64 codes in each of the 32 positions of a block, rows 0..4 (two 4-row groups), 66 blocks (two
   2048-wide K units, so two waves), scale bytes {2, 64, 120..134, 200, 252}; one-hot activations read every weight back.  Every output is
   value(code) * 2^(e - 127) bit for bit - which pins the bit order of the 192-bit operand, the split into a 16-byte and an 8-byte plane, the
   row interleave and the scale placement.  (The product row is a sum of one weight and K - 1 signed zeros, so a zero weight - code 0 or code
   32 - reads back as +0: IEEE addition of zeros of both signs.)  Under the smallest scale bytes the smallest elements are fp32 subnormals
   (0.125 * 2^-125): they are expected back exactly too.
2. `test_gemv_mx6_vs_fp64`: every compiled gemv_mx6 instantiation, reached through vv_linear_route and then vv_linear at the smallest k that
   selects it (whole units and ragged ends alternating), against a torch fp64 reference on the effective weights - the walk of
   tests/test_hip_gemv.py (whose case class, operand sets, layout with NaN gaps and guard rows, and three figures are imported): n in
   {1, 3, 4, 5, ...}, m in {1, 2}, broadcast rows, pitches wider than the rows, every prologue and epilogue, in-place residual, two runs
   bit-identical with every input bit-unchanged.  Cases with the "gemv_blocks" hook make one wave walk three and more row groups.
   Bars: that file's rule, checked on the CPU for every case here (`test_bars_sit_between_floor_and_dropped_chunk`): at least 8 x the error of
   an fp32 stand-in against fp64, at most a tenth of what one dropped 8-column chunk costs an element.  The rule admits the project's 3e-4 for
   every case, so BAR is that file's.  The effective weights are exact in fp32 and in the reference, as every other weight type's.
3. `test_built_unit_holds_exactly_the_enumerated_kernels` (CPU: reads the object file build() left): the gfx950 code object of
   vv_gemv_mx6.hip holds exactly the 32 enumerated kernels.
4. `test_refusals`: each refused argument set returns VV_E_UNSUPPORTED from vv_linear_route and from vv_linear, and nothing is written.
5. the engine: generate() against the oracle on mxfp6_effective_state_dict (bar 2e-2, the project's bar for this comparison in fp8, nf4 and
   mxfp4 modes) and not bit-equal to bf16, graphs equal eager, the decode step's recorded weight types, a batch of 3 on the lanes, and the
   7B-shape components (head sampling, prefill + batch-2 decode hidden state).
"""
import copy
import ctypes as C
import dataclasses
import functools
import math
import os
import zlib

import pytest
import torch

from conftest import rel_rms
from test_hip_gemv import BAR, DROP_MARGIN, EPS, FLOOR_HEADROOM, OPS, OPS_DUAL, Case, figures, fill_args, layout, route_of
from test_hip_mfma_gemm import _epilogue, _lib, _need_gpu, _prologue, _same_bits, built_kernels, instantiations_of
from test_hip_mxfp4 import _FAKE, _Tok, _gen, _special, _tuned

VV_E_UNSUPPORTED = -3
gpu = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------------------
# the kernel list and the decision, restated (vv_gemv_mx6.hip: VV_MX6_KERNELS, vv_gemv_mx6_decide)
# ---------------------------------------------------------------------------------------------------------------
UNIT = 2048                                              # one wave's 64 blocks of 32 k
SPLITS, LONG = (1, 2, 3, 4, 5, 6, 8), (10, 12)           # waves that split K; the long forms hold one weight stream only


def _mx6(m, dual, ksplit, ku):
    return f"gemv_mx6<m={m},dual={dual},ksplit={ksplit},ku={ku}>"


def mx6_exists(m, dual, ksplit, ku):
    return m in (1, 2) and ku == 1 and (ksplit in SPLITS or (not dual and ksplit in LONG))


ALL_MX6 = [_mx6(m, d, ks, 1) for m in (1, 2) for d in (0, 1) for ks in SPLITS + LONG if mx6_exists(m, d, ks, 1)]


def mx6_decide(m, k, dual):
    """the route name of an aligned call, or None (refused / longer than the kernels reach)"""
    if m > 2 or k % 32 or k > (8 if dual else 12) * UNIT:
        return None
    units = -(-k // UNIT)
    ksplit = units if units <= 6 else (units + 1) & ~1
    return _mx6(m, dual, ksplit, 1) if mx6_exists(m, dual, ksplit, 1) else None


NS = [37, 1, 33, 3, 4, 41, 5, 7, 50, 2]                  # n = 1, odd, a whole group, one past it, below the block's 4 waves (3)
TAILS = (32, 1056, 2016)                                 # ragged last units: whole 32-blocks


def _cases():
    cs = []

    def ops(dual, i, keep=lambda o: True):
        pool = [o for o in (OPS_DUAL if dual else OPS) if keep(o)]
        return dict(pool[i % len(pool)])

    def tag(o):
        return "_".join(filter(None, [o.get("pro", ""), "mod" if o.get("mod") else "", "b" if o.get("bias") else "", o.get("act", ""),
                                      {"chan": "gc", "row": "gr"}.get(o.get("gate"), ""), {"out": "res", "inplace": "inpl"}.get(o.get("res"), ""),
                                      "bcast" if o.get("ldx") == 0 else ""])) or "plain"

    reach = {}
    for m in (1, 2):
        for dual in (0, 1):
            for units in range(1, 14):
                inst = mx6_decide(m, units * UNIT, dual)
                if inst and inst not in reach:
                    reach[inst] = units
    assert set(reach) == set(ALL_MX6), sorted(set(reach) ^ set(ALL_MX6))
    assert mx6_decide(2, 12 * UNIT + 32, 0) is None and mx6_decide(2, 8 * UNIT + 32, 1) is None
    for i, inst in enumerate(ALL_MX6):
        f = dict(p.split("=") for p in inst[9:-1].split(","))
        m, dual, units = int(f["m"]), int(f["dual"]), reach[inst]
        k = units * UNIT if i % 2 == 0 else (units - 1) * UNIT + TAILS[(i // 2) % 3]
        n = NS[i % len(NS)]
        o = ops(dual, i, (lambda o: not o.get("gate")) if m * n == 1 else (lambda o: True))      # one output: no rms for a gate to stand on
        cs.append(Case(f"mx6_m{m}_d{dual}_ks{f['ksplit']}_n{n}_k{k}_{tag(o)}", inst, m, n, k, wq="mxfp6", **o))
    # the unit boundaries: one 32-block, the last block of a unit, one block into the next, 7 units on 8 waves, the longest rows of either kind,
    # 9 and 11 units on 10 and 12 waves
    for i, (k, dual) in enumerate(((32, 0), (32, 1), (2016, 0), (2080, 1), (6 * UNIT, 0), (6 * UNIT + 32, 0), (6 * UNIT + 32, 1), (8 * UNIT, 1),
                                   (12 * UNIT, 0), (8 * UNIT + 32, 0), (10 * UNIT + 32, 0))):
        for m in (1, 2):
            o = ops(dual, i + m)
            cs.append(Case(f"mx6_edge_m{m}_d{dual}_k{k}_{tag(o)}", mx6_decide(m, k, dual), m, 35, k, wq="mxfp6", **o))
    # a persistent grid: one block of 4 waves (or one K-split block) walks 3 and more row groups, the last one partial
    for i, (k, dual, n, blocks) in enumerate(((1024, 0, 61, 1), (1536, 1, 45, 1), (4096, 0, 27, 2), (6144, 1, 18, 1), (18944, 0, 13, 1))):
        o = ops(dual, i + 3)
        cs.append(Case(f"mx6_pers_d{dual}_k{k}_n{n}_{tag(o)}", mx6_decide(2, k, dual), 2, n, k, wq="mxfp6", hooks={"gemv_blocks": blocks}, **o))
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


# ---------------------------------------------------------------------------------------------------------------
# operands, the fp64 reference and the fp32 stand-in (CPU)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _weights(n, k, which):
    """(packed codes, packed scale bytes, the effective matrix) of one random [n, k] matrix"""
    from vibevoice_rocm_amd.weights import pack_mxfp6, quantize_mxfp6
    g = torch.Generator().manual_seed(zlib.crc32(repr((n, k, "mxfp6", which)).encode()))
    w = torch.randn(n, k, generator=g) / k ** 0.5
    codes, sbytes, eff = quantize_mxfp6(w.bfloat16())
    packed, sb = pack_mxfp6(codes, sbytes)
    return packed, sb, eff


@functools.lru_cache(maxsize=None)
def _operands_of(key):
    m, n, k, wq, pro, mod, bias, act, gate, res, bcast, _ = key
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    o = {"x": torch.randn(1 if bcast else m, k, generator=g)}
    o["w"], o["wscale"], o["w_eff"] = _weights(n, k, 0)
    if act == "swiglu":
        o["w2"], o["w2scale"], o["w2_eff"] = _weights(n, k, 1)
    if pro == "rms":
        o["norm_w"] = 1 + 0.1 * torch.randn(k, generator=g)
    if mod:
        o["shift"], o["scale"] = 0.2 * torch.randn(m, k, generator=g), 0.2 * torch.randn(m, k, generator=g)
    if bias:
        o["bias"] = 0.1 * torch.randn(n, generator=g)
    if gate == "chan":
        o["gate"] = torch.randn(n, generator=g)
    elif gate == "row":
        o["gate"] = torch.randn(m, n, generator=g)
    if res:
        o["res"] = torch.randn(m, n, generator=g)
    return o


def operands(case):
    return _operands_of(case.data_key)


def ref_fp64(case, o):
    x = _prologue(o["x"].expand(case.m, case.k), o, case.pro, torch.float64)
    y = x @ o["w_eff"].double().t()
    y2 = x @ o["w2_eff"].double().t() if "w2_eff" in o else None
    return _epilogue(y, y2, o, case.act, torch.float64)


@functools.lru_cache(maxsize=None)
def _expect_of(key, m, k, pro, act):
    """(fp64 reference, floor (global, row, element) of the fp32 stand-in, cost of one dropped 8-column K chunk): the rule of
    tests/test_hip_gemv.py (_expect_of), on this file's operands"""
    o = _operands_of(key)
    n = o["w_eff"].shape[0]
    ref = ref_fp64(Case("", "", m, n, k, pro=pro, act=act), o)
    xh = _prologue(o["x"].expand(m, k), o, pro, torch.float32)

    def chunks(w):      # fp32 partial products of the 8-column chunks, and their running sum in order
        P = torch.bmm(xh.reshape(m, k // 8, 8).transpose(0, 1), w.reshape(n, k // 8, 8).permute(1, 2, 0))
        return P, torch.cumsum(P, 0)[-1]

    P, acc = chunks(o["w_eff"])
    P2, acc2 = chunks(o["w2_eff"]) if "w2_eff" in o else (None, None)
    stand = _epilogue(acc, acc2, o, act, torch.float32).double()
    g, r, _, e, _ = figures(stand, ref)
    rms = math.sqrt(float((ref ** 2).mean()))
    d = _epilogue(acc[None] - P, acc2[None] - P2 if acc2 is not None else None, o, act, torch.float32).double() - stand
    return ref, (g, r, e), math.sqrt(float((d ** 2).mean())) / rms


def expect(case):
    return _expect_of(case.data_key, case.m, case.k, case.pro, case.act)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_bars_sit_between_floor_and_dropped_chunk(cid):
    """CPU only.  Both conditions on the class bar, for every case of this file: at least 8 x the fp32 stand-in's own error against the fp64
    reference (global, worst row, worst element), at most a tenth of what one dropped 8-column K chunk costs an element."""
    case = CASES[CASE_IDS.index(cid)]
    _, floor, drop = expect(case)
    bar = BAR[case.klass]
    print(f"{cid}: class {case.klass} bar {bar:.1e}  floor global {floor[0]:.2e} row {floor[1]:.2e} element {floor[2]:.2e}  dropped chunk {drop:.2e}")
    assert bar == 3e-4
    assert bar >= FLOOR_HEADROOM * max(floor), (cid, bar, floor)
    assert bar <= drop / DROP_MARGIN, (cid, bar, drop)


def test_cases_reach_every_compiled_instantiation():
    """CPU only: the enumerated set is 32 kernels, every one is some case's route, and the restated decision agrees with the library's on
    stand-in addresses for every case"""
    assert len(ALL_MX6) == len(set(ALL_MX6)) == 32
    assert {c.route for c in CASES} == set(ALL_MX6)
    for case in CASES:
        _, ld = layout(case, operands(case))
        with _tuned(case.hooks):
            assert route_of(_fill(case, ld, _FAKE)) == case.route, case.id


def test_built_unit_holds_exactly_the_enumerated_kernels(tmp_path):
    """What is compiled is what can launch (CPU only: reads the symbol table of the object file build() left): the gfx950 code object of
    vv_gemv_mx6.hip holds one gemv_mx6_kernel<m, dual, ksplit, ku> per entry of ALL_MX6, no other instantiation of the template and no other
    kernel."""
    built = built_kernels("vv_gemv_mx6.hip", tmp_path, plain=True)
    assert {k for k, _ in built} == {"gemv_mx6_kernel"}
    got = instantiations_of(built, {"gemv_mx6_kernel": _mx6})
    assert got == set(ALL_MX6), sorted(got ^ set(ALL_MX6))


# ---------------------------------------------------------------------------------------------------------------
# the call
# ---------------------------------------------------------------------------------------------------------------
def _fill(case, ld, ptr):
    """vv_lin_args of the case: test_hip_gemv's fill_args (which lays packed operands out as its NF4 cases') with the weight type set"""
    L = _lib()[0]
    shim = copy.copy(case)
    shim.wq = "nf4"
    a = fill_args(shim, ld, ptr)
    a.wdt = L.VV_MXFP6
    return a


_MEASURED = {}


def run_case(case):
    """Lay the case out (NaN in every pitch gap, two NaN guard rows behind the output), assert its route, launch it twice into separate outputs"""
    L, l = _lib()[:2]
    o = operands(case)
    buf, ld = layout(case, o)
    m, n, ldo = case.m, case.n, ld["ldo"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda() for _ in range(2)]
    with _tuned(case.hooks):
        for out in outs:
            a = _fill(case, ld, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
            got_route = route_of(a)
            assert got_route == case.route, (case.id, got_route, case.route)
            L.check(l.vv_linear(C.byref(a), None), "vv_linear")
        torch.cuda.synchronize()
    hs = [t.cpu() for t in outs]
    for name, t in dev.items():
        assert _same_bits(t.cpu(), buf[name]), f"{case.id}: input {name} was written"
    inside = torch.zeros(m + 2, ldo, dtype=torch.bool)
    inside[:m, :n] = True
    for i, h in enumerate(hs):
        grid = h.view(m + 2, ldo)
        assert torch.isfinite(grid[inside]).all(), f"{case.id}: run {i}: an in-range output is not finite"
        assert torch.isnan(grid[~inside]).all(), f"{case.id}: run {i}: a gap or guard element of out was written"
    assert _same_bits(hs[0], hs[1]), f"{case.id}: two runs of the same call differ"
    return hs[0].view(m + 2, ldo)[:m, :n].double()


@gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gemv_mx6_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    ref, floor, drop = expect(case)
    bar = BAR[case.klass]
    got = run_case(case)
    g, r, ri, e, ei = figures(got.numpy(), ref.numpy())
    print(f"{cid}: {case.route} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst row {r:.3e} (row {ri})  worst element {e:.3e} at {ei}  "
          f"[floor {max(floor):.2e}, dropped chunk {drop:.2e}]")
    mx = _MEASURED.setdefault(case.klass, [0.0, 0.0, 0.0])
    for i, v in enumerate((g, r, e)):
        mx[i] = max(mx[i], v)
    assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
    assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"
    assert e < bar, f"{cid}: element {ei} is {e:.3e} of the reference's rms from it, >= {bar:.1e}"


@gpu
def test_zz_report_and_hook_is_back_at_its_default():
    """the grid override is off again (a one-group-per-wave shape reports its route either way, so the check is the launch: n = 61 rows on
    the default grid), and the session's largest figures per class go where VV_MXFP6_PARITY_OUT says"""
    _need_gpu()
    run_case(Case("mx6_default_grid", mx6_decide(2, 1024, 0), 2, 61, 1024, wq="mxfp6", pro="rms", bias=True))
    path = os.environ.get("VV_MXFP6_PARITY_OUT")
    if path and _MEASURED:
        with open(path, "w") as f:
            f.write(f"{torch.cuda.get_device_name(0)}: largest figure against fp64 over each class's gemv_mx6 cases (tests/test_hip_mxfp6.py)\n")
            f.write(f"  {'class':<9} {'cases':>5} {'bar':>8} {'global':>10} {'row':>10} {'element':>10} {'bar / largest':>14}\n")
            for k, (g, r, e) in _MEASURED.items():
                f.write(f"  {k:<9} {sum(c.klass == k for c in CASES):>5} {BAR[k]:>8.1e} {g:>10.2e} {r:>10.2e} {e:>10.2e} {BAR[k] / max(g, r, e):>14.1f}\n")


# ---------------------------------------------------------------------------------------------------------------
# 1. decode, bit for bit
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_decode_is_exact():
    from vibevoice_rocm_amd.weights import MXFP6_VALUES, pack_mxfp6
    _need_gpu()
    L, l = _lib()[:2]
    n, k = 5, 2112                                                           # 66 blocks: one whole unit and two blocks of the next
    rows, cols = torch.arange(n)[:, None], torch.arange(k)[None, :]
    codes = ((cols + cols // 32 + 3 * rows) % 64).to(torch.uint8)           # code (33 j + i + 3 n) % 64 at k = 32 j + i: all 64 codes in every position
    for i in range(32):
        assert all(len(set(codes[r, i::32].tolist())) == 64 for r in range(n))
    pool = [2, 64] + list(range(120, 135)) + [200, 252]
    sbytes = torch.tensor(pool, dtype=torch.uint8)[(torch.arange(n * (k // 32)) * 7) % len(pool)].view(n, k // 32)      # 7 and 19 are coprime
    assert set(sbytes.reshape(-1).tolist()) == set(pool) and all(len(set(sbytes[r].tolist())) > 10 for r in range(n))
    val = torch.tensor(MXFP6_VALUES + tuple(-v for v in MXFP6_VALUES), dtype=torch.float64)
    want = (val[codes.long()] * torch.exp2(sbytes.double() - 127).repeat_interleave(32, dim=1))
    assert torch.isfinite(want.float()).all() and torch.equal(want.float().double(), want), "every expected weight is a finite fp32, exactly"
    want = want.float() + 0.0                                                # a zero weight reads back as +0 (docstring)
    packed, sb = [t.cuda() for t in pack_mxfp6(codes, sbytes)]
    x = torch.eye(k, device="cuda")
    for m in (1, 2):
        out = torch.full((k, n + 3), float("nan"), device="cuda")
        for k0 in range(0, k, m):
            a = L.LinArgs()
            a.x, a.ldx, a.m, a.n, a.k, a.wdt = x[k0].data_ptr(), k, m, n, k, L.VV_MXFP6
            a.w, a.wscale, a.out, a.ldo = packed.data_ptr(), sb.data_ptr(), out[k0].data_ptr(), n + 3
            if k0 == 0:
                assert route_of(a) == _mx6(m, 0, 2, 1)
            L.check(l.vv_linear(C.byref(a), None), "vv_linear")
        torch.cuda.synchronize()
        got = out.cpu()
        assert torch.isnan(got[:, n:]).all()
        got = got[:, :n].t().contiguous()                                    # [n, k]: W[n][k] as the kernel decoded it
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        assert bad.numel() == 0, (f"m={m}: {bad.shape[0]} of {n * k} weights differ; first (row, k) = {bad[0].tolist()}: got "
                                  f"{got[tuple(bad[0])].item()!r}, want {want[tuple(bad[0])].item()!r}, code {int(codes[tuple(bad[0])])}, "
                                  f"scale byte {int(sbytes[bad[0][0], bad[0][1] // 32])}")


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals():
    """m > 2, k % 32 != 0, a missing scale pointer (of w, of w2), a misaligned pointer (codes, scales), VV_LIN_W_FRAG, either bf16 hand-off
    flag and VV_LIN_W_MXGEMM: VV_E_UNSUPPORTED from vv_linear_route and from vv_linear alike, the output untouched; the same call without the
    fault runs."""
    from vibevoice_rocm_amd.weights import pack_mxfp6, quantize_mxfp6
    _need_gpu()
    L, l = _lib()[:2]
    n, k = 64, 1024
    c, s, _ = quantize_mxfp6(torch.randn(n, k + 32))
    p, q = [torch.cat([t, t]).cuda() for t in pack_mxfp6(c, s)]             # room behind every offset pointer below
    x = torch.randn(12, k + 32, device="cuda")
    out = torch.full((12, n), float("nan"), device="cuda")
    name = C.create_string_buffer(192)

    def args(m=2, kk=k, **kw):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo = x.data_ptr(), k + 32, m, n, kk, L.VV_MXFP6, out.data_ptr(), n
        a.w, a.wscale = p.data_ptr(), q.data_ptr()
        for f, v in kw.items():
            setattr(a, f, v)
        return a

    dual = dict(w2=p.data_ptr(), w2scale=q.data_ptr(), act=L.ACT_SWIGLU)
    refused = {"m=3": args(3), "m=12": args(12), "k%32": args(2, k + 16), "no wscale": args(wscale=None), "no w2scale": args(**{**dual, "w2scale": None}),
               "w+8": args(w=p.data_ptr() + 8), "wscale+2": args(wscale=q.data_ptr() + 2), "w2+8": args(**{**dual, "w2": p.data_ptr() + 8}),
               "w2scale+2": args(**{**dual, "w2scale": q.data_ptr() + 2}), "frag": args(flags=L.LIN_W_FRAG), "frag m=4": args(4, flags=L.LIN_W_FRAG),
               "x bf16": args(flags=L.LIN_X_BF16), "out bf16": args(flags=L.LIN_OUT_BF16), "x bf16 m=12": args(12, flags=L.LIN_X_BF16),
               "mxgemm": args(flags=L.LIN_W_MXGEMM), "mxgemm m=12 x bf16": args(12, flags=L.LIN_W_MXGEMM | L.LIN_X_BF16)}
    for what, a in refused.items():
        rc_route = l.vv_linear_route(C.byref(a), name, 192)
        rc_run = l.vv_linear(C.byref(a), None)
        assert rc_route == rc_run == VV_E_UNSUPPORTED, (what, rc_route, rc_run, l.vv_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its output"
    for a in (args(), args(1), args(**dual)):
        assert l.vv_linear_route(C.byref(a), name, 192) == 0 and name.value.decode().startswith("gemv_mx6<")
        assert l.vv_linear(C.byref(a), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out[:2]).all() and torch.isnan(out[2:]).all()


# ---------------------------------------------------------------------------------------------------------------
# 5. the engine at mid shapes, and the 7B widths
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("mid")
    seed = 4321
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, seed).items()}
    model = VibeVoiceForConditionalGenerationInference.from_synthetic(cfg, seed, device="cuda:0", torch_dtype=torch.bfloat16, numpy_weights=True,
                                                                      weight_quant="mxfp6")
    return cfg, sd, model


@gpu
def test_generate_mid_mxfp6_vs_oracle(mid):
    """from_synthetic(mid, weight_quant="mxfp6"): generate() (70-token prompt: prefill on the bf16 copies of the effective weights, decode on
    the MXFP6 codes) against the oracle on mxfp6_effective_state_dict under 2e-2; the same call in bf16 gives another waveform."""
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.weights import fp8_matrix_names, mxfp6_effective_state_dict
    cfg, sd, m = mid
    assert m.weight_quant == "mxfp6" and m.engine.w.quant == "mxfp6"
    eff = mxfp6_effective_state_dict(cfg, sd)
    names = set(fp8_matrix_names(cfg))
    sd_o = {k: (eff[k] if k in names else (v.to(torch.bfloat16).float() if v.dim() >= 2 else v)) for k, v in sd.items()}
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg.vocab - 8, (70,), generator=g)
    forced = [ST] + [D] * 5 + [E, EOS]
    noise = torch.randn(5, cfg.latent, generator=g)
    ref = O.generate(sd_o, cfg.as_dict(), ids.tolist(), torch.zeros(70, dtype=torch.bool), None, dict(speech_start=ST, speech_end=E,
                     speech_diffusion=D, eos=EOS), noise, cfg_scale=2.0, n_steps=10, forced_tokens=forced, bf16_t=True)
    out = _gen(m, cfg, ids, forced, noise)
    assert out.sequences[0, 70:].tolist() == forced
    got, want = out.speech_outputs[0][0].cpu().numpy(), torch.cat(ref.audio).numpy()
    assert got.shape == want.shape == (5 * cfg.hop,)
    err = rel_rms(got, want)
    m2 = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    plain = _gen(m2, cfg, ids, forced, noise).speech_outputs[0][0].cpu().numpy()
    far = rel_rms(plain, got)
    print(f"mxfp6 generate() vs oracle on the effective weights: rel RMS {err:.3e}; bf16 vs mxfp6: {far:.3e}")
    assert err < 2e-2, f"mxfp6 generate() vs oracle on the effective weights: rel RMS {err:.3e}"
    assert not (plain == got).all(), "the bf16 model gives the very same waveform: the test would pass on unquantised weights"


@gpu
def test_generate_mid_mxfp6_graphs_equal_eager(mid):
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg, sd, m = mid
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(12)
    ids = torch.randint(0, cfg.vocab - 8, (24,), generator=g)
    forced = [ST] + [D] * 4 + [E, ST, D, D, E, EOS]
    noise = torch.randn(6, cfg.latent, generator=g)
    eager = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", use_graphs=False)
    a, b = _gen(eager, cfg, ids, forced, noise).speech_outputs[0].cpu(), _gen(m, cfg, ids, forced, noise).speech_outputs[0].cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b), "mxfp6: graph replay must equal eager bit for bit"


@gpu
def test_decode_step_streams_mxfp6_for_every_companion_matrix(mid):
    """Under vv_prof_begin / vv_prof_end an eager generate() records, for every matrix that has a companion (fp8_matrix_names, K % 32 == 0), its
    m <= 2 launches with wdt == VV_MXFP6 - once per layer (and solver step) per decode step at least - and no launch of more than 2 rows with it."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg, sd, _ = mid
    L, l = _lib()[:2]
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(16)
    ids = torch.randint(0, cfg.vocab - 8, (70,), generator=g)
    forced = [ST, D, D, D, E, EOS]
    noise = torch.randn(3, cfg.latent, generator=g)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", use_graphs=False)
    _gen(m, cfg, ids, forced, noise)
    L.check(l.vv_prof_begin(100000), "vv_prof_begin")
    try:
        _gen(m, cfg, ids, forced, noise)
    finally:
        ents = (L.ProfEntry * 512)()
        cnt = C.c_int(0)
        L.check(l.vv_prof_end(ents, 512, C.byref(cnt)), "vv_prof_end")
    rec = [ents[i] for i in range(cnt.value)]
    mx = {(e.n, e.k, e.dual): e.count for e in rec if e.wdt == L.VV_MXFP6 and e.m <= 2}
    assert all(e.m <= 2 for e in rec if e.wdt == L.VV_MXFP6), "an MXFP6 launch with more than 2 rows"
    assert not any(e.wdt in (L.VV_FP8, L.VV_NF4, L.VV_MXFP4, L.VV_MXFP4_FRAG) for e in rec)
    steps, frames, decodes = 10, 3, len(forced) - 1                           # the first token after the prompt comes out of the prefill
    qkvd, hd = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, cfg.heads * cfg.head_dim
    c_dec, c_sem = cfg.ac_dec_filters * 2 ** len(cfg.ac_ratios), cfg.sem_filters * 2 ** len(cfg.sem_ratios)
    want = {}                                                                  # (n, k, dual) -> launches at least; matrices of one shape share a record
    for key, count in (((qkvd, cfg.hidden, 0), cfg.layers * decodes), ((cfg.hidden, hd, 0), cfg.layers * decodes),
                       ((cfg.inter, cfg.hidden, 1), cfg.layers * decodes), ((cfg.hidden, cfg.inter, 0), cfg.layers * decodes),
                       ((cfg.head_ffn, cfg.head_hidden, 1), cfg.head_layers * steps * frames),
                       ((cfg.head_hidden, cfg.head_ffn, 0), cfg.head_layers * steps * frames)):
        want[key] = want.get(key, 0) + count
    for (n, k, dual), least in want.items():
        assert k % 32 == 0
        assert mx.get((n, k, dual), 0) >= least, f"[{n}, {k}] dual={dual}: {mx.get((n, k, dual), 0)} MXFP6 launches with m <= 2, expected at least {least}"
    # the one-row conv stage's FFN matrices: whichever of their launches go through vv_linear at m <= 2 stream the companion (no other matrix
    # of the mid shapes is [4 C, C] or [C, 4 C])
    for c in (c_dec, c_sem):
        for n, k in ((4 * c, c), (c, 4 * c)):
            assert all(e.wdt == L.VV_MXFP6 for e in rec if (e.n, e.k) == (n, k) and e.m <= 2), f"[{n}, {k}]: a bf16 launch with m <= 2"


@gpu
def test_generate_mid_mxfp6_batch_of_3_on_lanes(mid):
    """3 mxfp6 dialogues run on the lock-step lanes (the row-batched path has no MXFP6) and equal three single-dialogue calls bit for bit;
    a serving session refuses the mode."""
    cfg, sd, m = mid
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(13)
    ids = torch.randint(0, cfg.vocab - 8, (3, 20), generator=g)
    forced = [[ST, D, D, D, E, EOS], [ST, D, E, EOS], [ST, D, D, E, ST, D, E, EOS]]
    noise = torch.randn(3, 4, cfg.latent, generator=g)
    m.set_ddpm_inference_steps(10)
    tok = _Tok(ST, E, D, EOS)
    out = m.generate(input_ids=ids, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    assert not m._rowbatch, "mxfp6 batch took the row-batched path"
    for b in range(3):
        one = m.generate(input_ids=ids[b:b + 1], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[b], noise=noise[b])
        assert torch.equal(one.speech_outputs[0].cpu(), out.speech_outputs[b].cpu()), f"dialogue {b}: lanes != single call"
    with pytest.raises(ValueError, match="weight_quant='mxfp6'"):
        m.open_session(tokenizer=tok, max_context=256)


@gpu
def test_7b_components_mxfp6_vs_oracle():
    """7B widths (H 3584, I 18944, head 3584 / 10752, untied lm_head; 2 LLM layers: the oracle runs on the CPU) with weight_quant="mxfp6": head
    sampling (20 steps, CFG 2), prompt prefill (70 rows, on the bf16 effective matrices) + one batch-2 decode step with the constrained logits,
    against the oracle on the effective weights under the 2e-2 bar of test_7b_components_mxfp4_vs_oracle."""
    _need_gpu()
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.engine import Engine
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    from vibevoice_rocm_amd.weights import mxfp6_effective_state_dict
    cfg = dataclasses.replace(VVConfig.preset("7b"), layers=2)
    sd = synth_state_dict_torch(cfg, 778, device="cuda:0", dtype=torch.bfloat16)
    torch.set_num_threads(16)
    eng = Engine(cfg, sd, device="cuda:0", dtype=torch.bfloat16, use_graphs=False, weight_quant="mxfp6")
    sd_o = mxfp6_effective_state_dict(cfg, sd)
    ocfg = cfg.as_dict()
    g = torch.Generator().manual_seed(42)

    def cpu(prefix):
        return {k: v.float().cpu() for k, v in sd_o.items() if k.startswith(prefix)}
    W = cpu("model.prediction_head.")
    cond, ncond, noise = torch.randn(1, cfg.hidden, generator=g), torch.randn(1, cfg.hidden, generator=g), torch.randn(1, cfg.latent, generator=g)
    ref = O.sample_speech_tokens(W, ocfg, cond, ncond, noise, 2.0, 20, bf16_t=True)[0].numpy()
    eng.set_steps(20)
    with torch.cuda.stream(eng.stream):
        eng.hidden2[0].copy_(cond[0].cuda()); eng.hidden2[1].copy_(ncond[0].cuda()); eng.noise_dev.copy_(noise[0].cuda())
        eng._ck(eng.lib.vv_head_sample(C.byref(eng.w.head), eng.hidden2.data_ptr(), cfg.hidden, eng.noise_dev.data_ptr(), eng.temb.data_ptr(),
                                       eng._coefs, 20, 2.0, eng.latent.data_ptr(), eng._head_ws.data_ptr(), None, eng.sp), "vv_head_sample")
    eng.stream.synchronize()
    e = rel_rms(eng.latent.cpu().numpy(), ref)
    assert e < 2e-2, f"7B mxfp6 head sampling: rel RMS {e:.3e}"
    del W
    W = cpu("model.language_model.")
    W["lm_head.weight"] = sd_o["lm_head.weight"].float().cpu()
    ids = torch.randint(0, 1000, (70,), generator=g)
    emb = W["model.language_model.embed_tokens.weight"]
    kv, nkv = O.KVCache(cfg.layers), O.KVCache(cfg.layers)
    h_ref = O.llm_forward(W, ocfg, emb[ids], kv, 0)[-1]
    O.llm_forward(W, ocfg, emb[ids[:7]], nkv, 0)
    valid = [cfg.vocab - 4, cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1]
    eng.begin_sequence(256, valid)
    eng.prefill(eng.embed_ids(ids), row=0)
    eng.prefill(eng.embed_ids(ids[:7]), row=1)
    eng.stream.synchronize()
    e = rel_rms(eng.hidden2[0].cpu().numpy(), h_ref.numpy())
    assert e < 2e-2, f"7B mxfp6 prefill(70) last hidden: rel RMS {e:.3e}"
    x = 0.05 * torch.randn(1, cfg.hidden, generator=g)
    p_ref = O.llm_forward(W, ocfg, x, kv, kv.length)[0]
    n_ref = O.llm_forward(W, ocfg, x, nkv, nkv.length)[0]
    with torch.cuda.stream(eng.stream):
        eng.x2[0].copy_(x[0].cuda()); eng.x2[1].copy_(x[0].cuda())
        eng.llm_forward(eng.x2, eng.lens, None, eng.hidden2)
        eng._logits()
    eng.stream.synchronize()
    ep, en = rel_rms(eng.hidden2[0].cpu().numpy(), p_ref.numpy()), rel_rms(eng.hidden2[1].cpu().numpy(), n_ref.numpy())
    assert ep < 2e-2 and en < 2e-2, f"7B mxfp6 batch-2 decode: positive {ep:.3e} negative {en:.3e}"
    lg_ref = (p_ref @ O.lm_head_weight(W, ocfg)[valid].t()).numpy()
    el = rel_rms(eng.logits[:4].cpu().numpy(), lg_ref)
    assert el < 2e-2, f"7B mxfp6 constrained logits: rel RMS {el:.3e}"
    eng.close()
