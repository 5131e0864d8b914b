"""The packed-prefill tile GEMM (csrc/vv_gemm_packed.hip, gemm_packed_kernel<dual, obf>) against the fp64 reference of tests/test_hip_mfma_gemm.py,
per 32 x 32 output tile - through the C ABI only.

The kernel is reached through VV_LIN_PACKED alone: the route tests (CPU) pin when the flag takes it and that every other call routes as without
the flag.  The parity grid puts M at 128, 129 and 300 rows (one full tile; one row in a second tile; three row tiles with a cut one) and at 9 rows
under vv_tune("gemm_packed_rows", 1), N at 128 and 384 (384 x 300 is 3 x 3 = 9 workgroups: a block remap that is not a bijection at
nwg % 8 != 0 drops or repeats a tile there) and K at 64, 128, 192 and 320: 1, 2, 3 and 5 steps of the two-buffer K loop - prologue only, one
hand-over, both buffers reused, and a drain.  Epilogues: plain, bias, residual in place, dual SwiGLU with a bf16 output.

Bars are BAR["xb"] (fp32 out) and BAR["bf16"] (bf16 out) of tests/test_hip_mfma_gemm.py, imported: bf16 operands are exact in the reference,
the kernel accumulates in fp32 and rounds a bf16 output once, as those classes do.  Layout, NaN gaps and guard rows, the two bit-identical runs
and the untouched inputs are that file's too.
"""
import ctypes as C

import pytest
import torch

from conftest import rel_rms
from test_hip_mfma_gemm import BAR, Case, _FAKE, _lib, _need_gpu, _same_bits, built_kernels, expect, fill_args, instantiations_of, layout, operands, \
    route_of, tile_row_errors

LIN_PACKED = 16


def _packed(dual, obf):
    return f"gemm_packed<dual={dual},obf={obf}>"


ALL_INSTANTIATIONS = [_packed(d, o) for d in (0, 1) for o in (0, 1)]

EPILOGUES = {"plain": dict(), "bias": dict(bias=True), "res_inplace": dict(res="inplace"), "swiglu_bf16out": dict(act="swiglu", out_bf16=True)}


def _cases():
    cs = []
    for m in (128, 129, 300, 9):
        for n in (128, 384):
            for k in (64, 128, 192, 320):
                for name, kw in EPILOGUES.items():
                    if m == 9 and (n, k) not in ((128, 64), (384, 320)):
                        continue               # the few-row form: the shortest and the longest loop
                    dual = int(kw.get("act") == "swiglu")
                    cs.append(Case(f"p_m{m}_n{n}_k{k}_{name}", _packed(dual, int(bool(kw.get("out_bf16")))), m, n, k, **kw))
    return cs


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


class _rows:
    """vv_tune("gemm_packed_rows", n) for a block; the default comes back afterwards (a negative value restores it)"""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        L, l = _lib()[:2]
        L.check(l.vv_tune(b"gemm_packed_rows", self.n), "vv_tune")

    def __exit__(self, *exc):
        L, l = _lib()[:2]
        L.check(l.vv_tune(b"gemm_packed_rows", -1), "vv_tune")


def _args(case, ptr, packed=True):
    a = fill_args(case, layout(case, operands(case))[1], ptr)
    if packed:
        a.flags |= LIN_PACKED
    return a


def test_flag_value_in_the_binding():
    L = _lib()[0]
    assert L.LIN_PACKED == LIN_PACKED


def test_route_takes_the_packed_kernel_only_where_it_is_meant_to():
    """CPU only (stand-in addresses, nothing launched).  With the flag, enough rows and a covered shape the route names gemm_packed<...>;
    without the flag, with n % 128 != 0, k % 64 != 0, an fp32 x, fewer rows than the threshold or the threshold at 0 it names exactly what the
    same call names without the flag."""
    plain = Case("r_plain", "", 300, 384, 192)
    dual = Case("r_dual", "", 300, 384, 192, act="swiglu", out_bf16=True)
    dual32 = Case("r_dual32", "", 300, 384, 192, act="swiglu")
    bias_res = Case("r_bias_res", "", 300, 384, 192, bias=True, res="out")
    with _rows(128):
        assert route_of(_args(plain, _FAKE)) == _packed(0, 0)
        assert route_of(_args(bias_res, _FAKE)) == _packed(0, 0)
        assert route_of(_args(dual, _FAKE)) == _packed(1, 1)
        assert route_of(_args(dual32, _FAKE)) == _packed(1, 0)
        for case in (plain, Case("r_n", "", 300, 448, 192), Case("r_k", "", 300, 384, 160), Case("r_f32", "", 300, 384, 192, xb=False),
                     Case("r_gelu", "", 300, 384, 192, act="gelu"), Case("r_gate", "", 300, 384, 192, gate="chan"), Case("r_few", "", 127, 384, 192)):
            today = route_of(_args(case, _FAKE, packed=False))
            assert not today.startswith("gemm_packed"), (case.id, today)
            if case is not plain:
                assert route_of(_args(case, _FAKE)) == today, case.id
        misaligned = dict(_FAKE, bias=_FAKE["bias"] + 4)           # a bias the vector epilogue cannot load: today's kernel and its scalar epilogue
        case = Case("r_bias4", "", 300, 384, 192, bias=True)
        assert route_of(_args(case, misaligned)) == route_of(_args(case, misaligned, packed=False))
    with _rows(0):
        assert route_of(_args(plain, _FAKE)) == route_of(_args(plain, _FAKE, packed=False))
    with _rows(1):
        assert route_of(_args(Case("r_9", "", 9, 128, 64), _FAKE)) == _packed(0, 0)


@pytest.mark.parametrize("cid", CASE_IDS)
def test_route_of_every_case_on_the_host(cid):
    case = CASES[CASE_IDS.index(cid)]
    with _rows(1 if case.m < 128 else 128):
        assert route_of(_args(case, _FAKE)) == case.route


def test_built_library_holds_exactly_the_enumerated_kernels(tmp_path):
    """vv_gemm_packed.hip's gfx950 code object holds the four instantiations of gemm_packed_kernel and no other (CPU only: symbol names of
    the object file build() left)"""
    got = instantiations_of(built_kernels("vv_gemm_packed.hip", tmp_path), {"gemm_packed_kernel": _packed})
    assert got == set(ALL_INSTANTIATIONS), sorted(got ^ set(ALL_INSTANTIATIONS))


def _run(case):
    """test_hip_mfma_gemm.run_case with VV_LIN_PACKED set: two launches into separate outputs, bit-identical; NaN gaps and guards intact"""
    L, l = _lib()[:2]
    buf, ld = layout(case, operands(case))
    m, n, ldo = case.m, case.n, ld["ldo"]
    dev = {name: t.cuda() for name, t in buf.items() if name != "out"}
    outs = [buf["out"].cuda(), buf["out"].cuda()]
    with _rows(1 if m < 128 else 128):
        for out in outs:
            a = _args(case, {**{name: t.data_ptr() for name, t in dev.items()}, "out": out.data_ptr()})
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
    return grid[:m, :n].double()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", CASE_IDS)
def test_gemm_packed_vs_fp64(cid):
    _need_gpu()
    case = CASES[CASE_IDS.index(cid)]
    ref = expect(case)[0]
    got = _run(case).numpy()
    g = rel_rms(got, ref.numpy(), f"{cid} [{case.route}] global")
    t, ti, r, ri = tile_row_errors(got, ref.numpy())
    bar = BAR[case.klass]
    print(f"{cid}: {case.route} class {case.klass} bar {bar:.1e}  global {g:.3e}  worst tile {t:.3e} at (row tile {ti[0]}, channel tile {ti[1]})  "
          f"worst row {r:.3e} (row {ri})")
    assert g < bar, f"{cid}: global rel RMS {g:.3e} >= {bar:.1e}"
    assert t < bar, f"{cid}: 32 x 32 tile (row tile {ti[0]}, channel tile {ti[1]}) rel RMS {t:.3e} >= {bar:.1e}"
    assert r < bar, f"{cid}: row {ri} rel RMS {r:.3e} >= {bar:.1e}"


@pytest.mark.gpu
def test_zz_threshold_is_back_at_its_default():
    """a leaked vv_tune("gemm_packed_rows") would change what the flag does for every later test: under the default and under an explicit
    restore the same call reports the same route"""
    _need_gpu()
    L, l = _lib()[:2]
    case = Case("h", "", 300, 384, 192)
    now = route_of(_args(case, _FAKE))
    L.check(l.vv_tune(b"gemm_packed_rows", -1), "vv_tune")
    assert route_of(_args(case, _FAKE)) == now
