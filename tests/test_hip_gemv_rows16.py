"""gemv_rows16_kernel (csrc/vv_gemv_rows.hip): the matrix-core GEMV for 9 .. 16 activation rows on fragment-major bf16 weights, against fp64.

The machinery is tests/test_hip_gemv.py's: Case, operands, the NaN-gapped layout, ref_fp64 (activations rounded once to bf16 hi + lo, as the rows
classes there), the three figures (global, worst row, worst element) and the class bars BAR["rows"] / BAR["rows_rms"] = 3e-4, whose derivation
(the hi / lo arithmetic and the fp32 sum, K <= 8256) does not depend on the row count.  test_bars_sit_between_floor_and_dropped_chunk holds the
cases of this file to the same two conditions on the CPU.

Cases: each of the 12 compiled instantiations at the smallest k that selects it under the case's vv_tune settings (test_cases_cover_the_
instantiations checks both), with m = 9 (one row in the second tile), 12 and 16; n = 16 (one row group) and several groups; ragged last k steps
(a wave with fewer loads than the others, waves with none); plain, RMSNorm and RMSNorm + adaLN prologues; bias, GELU, SwiGLU, row gate, channel
gate, residual, in place; ldx = k + 8 everywhere.  What the fragment-major layout rules out is refused instead (test_refused): n that is no
multiple of 16 (so no n below the wave count either) and broadcast rows (ldx = 0), which the 8-row kernel declines too.

Every case runs twice, bit for bit (the atomic form: each run to the bar), the ticket forms a third time (the tickets were left zero); gaps and
guards stay NaN, inputs unchanged.  Row independence: a permutation of the input rows permutes the output rows bit for bit (whole-row and ticket
forms), and rows 0 .. 7 of the call equal gemv_rows_kernel's output on those 8 rows - bit for bit wherever both launchers cut K alike, which is
every case here but the two of CUT_DIFFERS, one row group each, where the 8-row launcher takes 10 K slices and the 16-row one, which has at most
8, takes fewer and longer ones (r16_s12: 10 slices of 3 loads against 3 of 10; r16_cut_differs, under gemv_rows_blocks = 10: 10 of 5 against 5
of 10): those two are held to the bar, and so is the atomic case.  test_cut_differs_names_the_shapes keeps that list true on the CPU."""
import ctypes as C
import os
import sys

import pytest
import torch

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_hip_gemv import (BAR, DROP_MARGIN, FLOOR_HEADROOM, Case, _tuned, expect, figures, fill_args, layout, operands, route_of)
from test_hip_mfma_gemm import _FAKE, _lib, _need_gpu, _same_bits, built_kernels, instantiations_of

ROWS16_FORMS = [(0, 8, 4, 0), (0, 8, 6, 0), (0, 8, 8, 0), (1, 8, 4, 0), (1, 8, 6, 0), (1, 8, 8, 0), (1, 8, 4, 1), (1, 8, 6, 1),
                (0, 4, 3, 0), (0, 4, 6, 0), (0, 4, 9, 0), (0, 4, 12, 0)]


def _rows16(dual, nw, ks, pers):
    return f"gemv_rows16<dual={dual},nw={nw},ks={ks},pers={pers}>"


ALL_ROWS16 = [_rows16(*f) for f in ROWS16_FORMS]


def decide(m, n, k, dual, mod, atomic_ok, tune):
    """vv_gemv_rows_decide for bf16 fragment-major weights with the process-wide scratch on, aligned operands, 3 <= m <= 16:
    (kernel name, nw, ksplit, loads per wave, atomic) or None.  9 .. 16 rows: at most 8 K slices (the partial tiles are twice the size)."""
    pers_cap, blocks = tune.get("gemv_rows_pers", 192), tune.get("gemv_rows_blocks", 448)
    if not 3 <= m <= 16 or k % 32 or k < 32 or n % 16:
        return None
    wide = m > 8
    name = (lambda d, nw, ks, p: _rows16(d, nw, ks, p)) if wide else (lambda d, nw, ks, p: f"gemv_rows<dual={d},nw={nw},ks={ks},pers={p},f8=0>")
    steps, groups = k // 32, n // 16
    if k <= 2048:
        spw = -(-steps // 8)
        ks = 4 if spw <= 4 else 6 if spw <= 6 else 8
        return name(dual, 8, ks, int(bool(dual) and groups > pers_cap and spw <= 6)), 8, 1, spw, 0
    if mod:
        return None
    nw = 8 if dual else 4
    kscap, ksmax, few = (8, 8, 3) if dual else (9, 12, 3)
    top = 8 if wide else 16
    per = lambda sp: -(-steps // (sp * nw))
    pick = next((sp for sp in range(2, top + 1) if per(sp) <= kscap and (groups * sp >= blocks or per(sp) <= few)), None)
    if not pick:
        pick = next((sp for sp in range(2, top + 1) if per(sp) <= ksmax), None)
    if not pick:
        return None
    spw, ksplit = per(pick), pick
    while ksplit > 1 and (ksplit - 1) * nw * spw >= steps:
        ksplit -= 1
    atomic = int(bool(tune.get("gemv_rows_atomic", 1)) and not dual and atomic_ok)
    ks = next(s for s in ((4, 6, 8) if dual else (3, 6, 9, 12)) if spw <= s)
    return name(dual, nw, ks, 0), nw, ksplit, spw, atomic


S = {"gemv_rows_scratch": 1}
B1, B6, P3 = {"gemv_rows_blocks": 1}, {"gemv_rows_blocks": 6}, {"gemv_rows_pers": 3}


def _atomic_ok(dual, o):
    return not dual and o.get("pro", "none") == "none" and o.get("act", "none") == "none" and o.get("res") == "inplace"


def _case(cid, m, n, k, dual, hooks=None, want=None, **o):
    hooks = {**S, **(hooks or {})}
    o = {**({"act": "swiglu"} if dual else {}), **o}
    inst, nw, ksplit, spw, atomic = decide(m, n, k, dual, o.get("mod", False), _atomic_ok(dual, o), hooks)
    assert want is None or inst == _rows16(*want), (cid, inst, want)
    c = Case(cid, inst, m, n, k, frag=True, hooks=hooks, suffix=f" ksplit={ksplit} atomic={atomic}", runs=2 if ksplit == 1 or atomic else 3, **o)
    c.cut = (nw, ksplit, spw)
    return c


def _cases():
    cs = [
        # whole rows (k <= 2048): 8 waves, 4 / 6 / 8 loads per wave
        _case("r16_w4_k32_one_step", 9, 16, 32, 0, want=(0, 8, 4, 0)),                                     # one k step: seven waves have none
        _case("r16_w4_ragged", 12, 48, 1024 - 32, 0, want=(0, 8, 4, 0), pro="rms", bias=True),
        _case("r16_w6", 16, 32, 33 * 32, 0, want=(0, 8, 6, 0), pro="rms", mod=True, gate="row", res="inplace"),
        _case("r16_w8", 9, 32, 49 * 32, 0, want=(0, 8, 8, 0), bias=True, act="gelu", gate="chan", res="out"),
        _case("r16_w8_full", 16, 16, 2048, 0, want=(0, 8, 8, 0), pro="rms_now", gate="row", res="out"),
        _case("r16_d_w4", 12, 16, 32, 1, want=(1, 8, 4, 0), pro="rms", mod=True),
        _case("r16_d_w4_k1024", 9, 32, 1024, 1, want=(1, 8, 4, 0), gate="row", res="out"),
        _case("r16_d_w6", 9, 32, 33 * 32, 1, want=(1, 8, 6, 0), pro="rms_now", gate="row", res="out"),
        _case("r16_d_w8", 16, 32, 49 * 32, 1, want=(1, 8, 8, 0), pro="rms"),
        _case("r16_d_w8_full", 12, 16, 2048, 1, want=(1, 8, 8, 0), pro="rms", mod=True, gate="chan"),
        # persistent: seven row groups over three blocks (3 + 2 + 2 groups)
        _case("r16_d_p4_7groups", 16, 112, 32, 1, P3, want=(1, 8, 4, 1), pro="rms", mod=True),
        _case("r16_d_p4_7groups_k544", 9, 112, 512 + 32, 1, P3, want=(1, 8, 4, 1), res="inplace"),
        _case("r16_d_p6_7groups", 12, 112, 33 * 32, 1, P3, want=(1, 8, 6, 1), pro="rms", gate="chan", res="out"),
        _case("r16_d_p6_7groups_mod", 16, 112, 1536, 1, P3, want=(1, 8, 6, 1), pro="rms", mod=True, gate="row"),
        # K slices folded through the ticket: 4 waves, 3 / 6 / 9 / 12 loads per wave
        _case("r16_s3", 12, 32, 65 * 32, 0, want=(0, 4, 3, 0), pro="rms", bias=True, res="out"),
        _case("r16_s6", 16, 32, 65 * 32, 0, B6, want=(0, 4, 6, 0), bias=True, act="gelu"),
        _case("r16_s9", 9, 32, 65 * 32, 0, B1, want=(0, 4, 9, 0), pro="rms_now", gate="row", res="inplace"),
        _case("r16_s12", 12, 16, 109 * 32, 0, want=(0, 4, 12, 0), pro="rms", bias=True),
        _case("r16_s12_k8256", 16, 16, 8256, 0, want=(0, 4, 12, 0), gate="chan", res="out"),
        # SwiGLU K slices: 8 waves
        _case("r16_d_s4", 9, 32, 65 * 32, 1, want=(1, 8, 4, 0), pro="rms"),
        _case("r16_d_s6", 16, 32, 65 * 32, 1, B1, want=(1, 8, 6, 0), pro="rms", gate="row", res="out"),
        _case("r16_d_s8", 12, 32, 97 * 32, 1, B1, want=(1, 8, 8, 0)),
        # the in-place linear epilogue: K slices add into out (atomic), or through the ticket
        _case("r16_inplace_atomic", 16, 32, 65 * 32, 0, bias=True, gate="row", res="inplace"),
        _case("r16_inplace_ticket", 16, 32, 65 * 32, 0, {"gemv_rows_atomic": 0}, bias=True, gate="row", res="inplace"),
        # one row group, ten blocks asked for: the 8-row launcher cuts K ten ways, this one five
        _case("r16_cut_differs", 16, 16, 200 * 32, 0, {"gemv_rows_blocks": 10}, want=(0, 4, 12, 0), pro="rms", bias=True),
    ]
    assert len({c.id for c in cs}) == len(cs)
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]
CUT_DIFFERS = ("r16_s12", "r16_cut_differs")             # the 8-row launcher cuts K into other slices than the 16-row one


def _by_id(cid):
    return CASES[CASE_IDS.index(cid)]


def _case8(case):
    """the case's first 8 rows as a call of gemv_rows_kernel (same shape, operands kinds and settings), and whether both launchers cut K alike"""
    ops = dict(pro=case.pro, mod=case.mod, bias=case.bias, act=case.act, gate=case.gate, res=case.res)
    inst, nw, ksplit, spw, atomic = decide(8, case.n, case.k, case.dual, case.mod, _atomic_ok(case.dual, ops), case.hooks)
    c8 = Case(case.id + "_8", inst, 8, case.n, case.k, frag=True, hooks=case.hooks, suffix=f" ksplit={ksplit} atomic={atomic}", runs=1, **ops)
    return c8, (nw, ksplit, spw) == case.cut


# ---------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------
def test_cut_differs_names_the_shapes():
    assert {c.id for c in CASES if not _case8(c)[1]} == set(CUT_DIFFERS)


def test_cases_cover_the_instantiations():
    """every instantiation is reached, and by a case at the smallest k (a multiple of 32) that selects it under that case's settings"""
    assert {c.route for c in CASES} == set(ALL_ROWS16)
    for inst in ALL_ROWS16:
        smallest = []
        for c in (c for c in CASES if c.route == inst):
            o = dict(mod=c.mod, pro=c.pro, act=c.act, res=c.res)
            k0 = next(k for k in range(32, 8257, 32) if (decide(c.m, c.n, k, c.dual, c.mod, _atomic_ok(c.dual, o), c.hooks) or [None])[0] == inst
                      and (k <= 2048) == (c.k <= 2048))
            smallest.append(c.k == k0)
        assert any(smallest), inst
    assert {c.m for c in CASES} == {9, 12, 16} and max(c.k for c in CASES) <= 8256


@pytest.mark.parametrize("cid", CASE_IDS)
def test_bars_sit_between_floor_and_dropped_chunk(cid):
    """the two conditions of tests/test_hip_gemv.py on the class bar, for the cases of this file (CPU only)"""
    case = _by_id(cid)
    _, floor, drop = expect(case)
    bar = BAR[case.klass]
    print(f"{cid}: class {case.klass} bar {bar:.1e}  floor global {floor[0]:.2e} row {floor[1]:.2e} element {floor[2]:.2e}  dropped chunk {drop:.2e}")
    assert bar >= FLOOR_HEADROOM * max(floor), (cid, bar, floor)
    assert bar <= drop / DROP_MARGIN, (cid, bar, drop)


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """the gfx950 code object of vv_gemv_rows.hip holds the 12 gemv_rows16_kernel instantiations of ROWS16_FORMS and no other (symbol names only)"""
    got = instantiations_of(built_kernels("vv_gemv_rows.hip", tmp_path), {"gemv_rows16_kernel": _rows16})
    assert got == set(ALL_ROWS16), sorted(got ^ set(ALL_ROWS16))


def test_without_scratch_the_fragment_major_call_is_refused_on_the_host():
    """CPU only (stand-in addresses, nothing is launched): 9 rows on VV_LIN_W_FRAG weights need the split-K scratch, as 3 .. 8 rows do"""
    L, l = _lib()[:2]
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo, a.flags = _FAKE["x"], 1024, 9, 32, 1024, L.VV_BF16, _FAKE["w"], _FAKE["out"], 32, L.LIN_W_FRAG
    name = C.create_string_buffer(192)
    assert l.vv_linear_route(C.byref(a), name, 192) != 0 and "FRAG" in l.vv_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------
def launch(case, o, want_route=True):
    """Lay the case out on operands o, assert its route, launch it case.runs times into separate outputs; checks repeatability, gaps, guards and
    inputs; returns (the runs' out[m, n] as fp32 tensors - one if they are bit-identical -, the route name)"""
    L, l = _lib()[:2]
    buf, ld = layout(case, o)
    m, n, ldo = case.m, case.n, ld["ldo"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda() for _ in range(case.runs)]
    with _tuned(case.hooks):
        for out in outs:
            a = fill_args(case, ld, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
            route = route_of(a)
            assert not want_route or route == case.name, (case.id, route, case.name)
            L.check(l.vv_linear(C.byref(a), None), "vv_linear")
        torch.cuda.synchronize()
    hs = [t.cpu() for t in outs]
    for name, t in dev.items():
        assert _same_bits(t.cpu(), buf[name]), f"{case.id}: input {name} was written"
    inside = torch.zeros(m + 2, ldo, dtype=torch.bool)
    inside[:m, :n] = True
    for i, h in enumerate(hs):
        grid = h.view(m + 2, ldo)
        assert torch.isfinite(grid[inside]).all(), f"{case.id}: run {i}: in-range outputs are not finite"
        assert torch.isnan(grid[~inside]).all(), f"{case.id}: run {i}: a gap or guard element of out was written"
    got = [h.view(m + 2, ldo)[:m, :n].clone() for h in hs]
    if route.endswith("atomic=1"):
        return got, route
    for i, h in enumerate(got[1:]):
        assert _same_bits(got[0], h), f"{case.id}: run {i + 1} of the same call differs from run 0"
    return got[:1], route


def _rows_of(o, m, idx):
    """the operand set with its per-row arrays (activations, adaLN rows, row gate, residual) taken at rows idx"""
    out = dict(o)
    for name in ("x", "shift", "scale", "res"):
        if name in o:
            out[name] = o[name][idx].contiguous()
    if "gate" in o and o["gate"].dim() == 2:
        out["gate"] = o["gate"][idx].contiguous()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_rows16_vs_fp64(cid):
    _need_gpu()
    case = _by_id(cid)
    ref, floor, drop = expect(case)
    bar = BAR[case.klass]
    outs, _ = launch(case, operands(case))
    for got in outs:
        g, r, ri, e, ei = figures(got.double().numpy(), ref.numpy())
        print(f"{cid}: {case.name} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst row {r:.3e} (row {ri})  worst element {e:.3e} at {ei}  "
              f"[floor {max(floor):.2e}, dropped chunk {drop:.2e}]")
        assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
        assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"
        assert e < bar, f"{cid}: element {ei} is {e:.3e} of the reference's rms from it, >= {bar:.1e}"


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in CASES if not c.name.endswith("atomic=1")])
def test_permuted_rows_give_permuted_rows(cid):
    """whole-row and ticket forms: the rows do not see each other, whichever tile and fragment row they sit in"""
    _need_gpu()
    case = _by_id(cid)
    o = operands(case)
    perm = torch.randperm(case.m, generator=torch.Generator().manual_seed(case.m * 1000 + case.n))
    assert not torch.equal(perm, torch.arange(case.m))
    (a,), _ = launch(case, o)
    (b,), _ = launch(case, _rows_of(o, case.m, perm))
    assert _same_bits(a[perm], b), f"{cid}: output rows of the permuted call are not the permuted output rows"


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_first_tile_equals_the_8_row_kernel(cid):
    """rows 0 .. 7 against gemv_rows_kernel on those 8 rows, same weights and settings: bit for bit where both cut K alike, else within the bar"""
    _need_gpu()
    case = _by_id(cid)
    o = operands(case)
    c8, alike = _case8(case)
    outs16, _ = launch(case, o)
    outs8, _ = launch(c8, _rows_of(o, case.m, torch.arange(8)))
    assert alike == (cid not in CUT_DIFFERS)
    if alike and not case.name.endswith("atomic=1"):
        assert _same_bits(outs16[0][:8], outs8[0]), f"{cid}: rows 0..7 differ from the 8-row kernel's"
    else:
        ref = expect(case)[0][:8]
        for got in (outs16[0][:8], outs8[0]):
            g, r, _, e, _ = figures(got.double().numpy(), ref.numpy())
            assert max(g, r, e) < BAR[case.klass], (cid, g, r, e)


@pytest.mark.gpu
def test_refused():
    """VV_LIN_W_FRAG calls the 16-row kernel does not take stay errors that name FRAG: 17 rows, fp8 codes at 9 rows, a long K without scratch (and
    past 8 slices with it), n that is no multiple of 16, broadcast rows"""
    _need_gpu()
    L, l = _lib()[:2]
    x = torch.randn(17, 12320 + 8, device="cuda")
    w = torch.zeros(32 * 12320, dtype=torch.bfloat16, device="cuda")
    sc = torch.ones(32, device="cuda")
    out = torch.zeros(17, 36, device="cuda")

    def call(m, n, k, wdt=None, scratch=0, ldx=None, text="FRAG"):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo = x.data_ptr(), k + 8 if ldx is None else ldx, m, n, k, L.VV_BF16 if wdt is None else wdt, w.data_ptr(), out.data_ptr(), 36
        a.flags = L.LIN_W_FRAG
        if wdt is not None:
            a.wscale = sc.data_ptr()
        with _tuned({"gemv_rows_scratch": scratch}):
            rc = l.vv_linear(C.byref(a), None)
            err = l.vv_last_error().decode()
        assert rc != 0 and text in err, (m, n, k, rc, err)

    call(17, 32, 1024, scratch=1)
    call(9, 32, 1024, wdt=L.VV_FP8, scratch=1)
    call(9, 32, 65 * 32)                        # K slices, no scratch
    call(9, 32, 12320, scratch=1)               # 385 loads: more than 8 slices of 4 x 12
    call(9, 24, 1024, scratch=1)
    call(9, 32, 1024, scratch=1, ldx=0, text="broadcast rows")      # ldx = 0 past 8 rows: an argument error of vv_linear itself
    torch.cuda.synchronize()
    assert torch.count_nonzero(out) == 0
