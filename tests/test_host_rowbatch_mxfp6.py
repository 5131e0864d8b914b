"""CPU tests of MXFP6 on the row-batched decode path (weight_quant="mxfp6", mxfp6_row_batch=True; csrc/vv_gemv_rows_mx6.hip):
the fragment-major VV_MXFP6_FRAG packing against the header's layout sentence, its inverse, the shapes it refuses; the decision's rules
restated, the kernel set of the built unit, the route vv_linear_route names for the cases of tests/test_hip_rowbatch_mxfp6.py and every refusal
(stand-in addresses: nothing is launched, no pointer is followed); the opt-in keyword, the descriptor bit and the fragment copies ensure_frag
builds (on the CPU, at `tiny`).

What a host without a GPU cannot ask: vv_linear takes a K split that folds through tickets only with the process-wide split-K scratch, which is
device memory (vv_tune("gemv_rows_scratch", 1)).  Here the K-split cases are therefore asked in their in-place form (the atomic split needs no
scratch: the same instantiation, the same cut) or shown to be refused without scratch; the GPU file asserts the ticketed route of every case."""
import ctypes as C
import dataclasses
import os
import re

import pytest
import torch

from test_hip_mfma_gemm import built_kernels, instantiations_of
from test_host_rowbatch_mxfp4 import _split
from vibevoice_rocm_amd import _lib
from vibevoice_rocm_amd.weights import DeviceWeights, unpack_mxfp6

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VV_E_UNSUPPORTED = -3


# ---------------------------------------------------------------------------------------------------------------
# the decision's rules, restated (vv_gemv_rows.hip: vv_gemv_rows_decide on VV_MXFP6_FRAG weights)
# ---------------------------------------------------------------------------------------------------------------
def _mx6(dual, nw, ks, pers):
    return f"gemv_rows_mx6<dual={dual},nw={nw},ks={ks},pers={pers}>"


# every kernel of the unit (gemv_rows_mx6_kernel<dual, nw, ks, pers>): whole rows (8 waves, 1 or 2 loads of 128 k per wave; SwiGLU also
# persistent), the SwiGLU K split (the same two one-shot kernels), the single-matrix K split (4 waves, 1..4 loads)
ALL_ROWS_MX6 = [_mx6(0, 8, 1, 0), _mx6(0, 8, 2, 0), _mx6(1, 8, 1, 0), _mx6(1, 8, 2, 0), _mx6(1, 8, 1, 1), _mx6(1, 8, 2, 1),
                _mx6(0, 4, 1, 0), _mx6(0, 4, 2, 0), _mx6(0, 4, 3, 0), _mx6(0, 4, 4, 0)]


def rows_mx6_decide(n, k, dual, mod=False, blocks=448, pers=192, atomic=False):
    """(route name as vv_linear_route prints it, K cut (waves, 128-wide loads per wave, K slices)) of an aligned 3..8-row VV_MXFP6_FRAG call with
    split-K scratch (or, atomic, in its in-place form), or None (not covered).  A load is 128 k, as for VV_MXFP4_FRAG: four A fragments per load
    bound the loads per wave to 2 in the 8-wave kernels and 4 in the 4-wave K split."""
    if n % 16 or k % 128:
        return None
    steps, n_groups = k // 128, n // 16
    if steps <= 16:                                    # K <= 2048: whole rows, no cross-block reduction
        spw = (steps + 7) // 8
        p = int(bool(dual) and n_groups > pers)
        return f"{_mx6(int(dual), 8, spw, p)} ksplit=1 atomic=0", (8, spw, 1)
    if mod:                                            # the modulated prologue needs the whole row's statistic up front
        return None
    nw = 8 if dual else 4
    cut = _split(steps, n_groups, nw, 2 if dual else 3, 2 if dual else 4, 1, blocks)
    if cut is None:
        return None
    ksplit, spw = cut
    return f"{_mx6(int(dual), nw, spw, 0)} ksplit={ksplit} atomic={int(atomic and not dual)}", (nw, spw, ksplit)


# The cases of the GPU file: (n, k, dual, rms prologue, adaLN, gate + residual epilogue (else bias), hooks) - the smallest shapes that reach
# every instantiation in every form.  The decision is MXFP4's (the same load width), so the list is tests/test_hip_rowbatch_mxfp4.py's
CASES = {
    "one_load_k128": (32, 128, 0, 0, 0, 1, {}),                           # one load per wave, wave 0 alone
    "one_load_k384_ragged": (32, 384, 0, 1, 0, 0, {}),                    # three of eight waves live
    "whole_row_k2048": (32, 2048, 0, 1, 0, 0, {}),                        # the widest whole-row slice: two loads per wave
    "dual_k512": (48, 512, 1, 1, 0, 0, {}),
    "dual_adaln_k1536": (48, 1536, 1, 1, 1, 0, {}),                       # SwiGLU with the adaLN prologue, two loads, waves 6 and 7 idle
    "dual_pers_k1024": (80, 1024, 1, 1, 1, 0, {"gemv_rows_pers": 2}),     # two persistent blocks walk 3 and 2 row groups
    "dual_pers_k2048": (80, 2048, 1, 1, 0, 0, {"gemv_rows_pers": 2}),
    "split_k2176_ragged": (48, 2176, 0, 0, 0, 1, {}),                     # 5 slices of 4 loads, the last holds one
    "split_k4608_rms": (48, 4608, 0, 1, 0, 1, {}),                        # 9 slices; the RMS statistic meets through the partial tiles
    "split_ks2_k4608": (48, 4608, 0, 0, 0, 1, {"gemv_rows_blocks": 15}),  # 5 slices of 2 loads per wave, the last ragged
    "split_ks3_k4608": (48, 4608, 0, 1, 0, 0, {"gemv_rows_blocks": 9}),   # 3 slices of 3 loads per wave
    "split_ks4_k18944": (32, 18944, 0, 0, 0, 1, {}),                      # the 7B down projection's K: 10 slices of 4 loads, the last ragged
    "dual_split_k2176": (32, 2176, 1, 1, 0, 0, {}),                       # SwiGLU K split: 3 slices, the last holds one load
    "dual_split_ks2_k3584": (32, 3584, 1, 1, 0, 0, {"gemv_rows_blocks": 1}),   # the 7B gate / up cut: 2 slices of 2 loads per wave
}


def route_of_case(case, atomic=False):
    n, k, dual, pro, mod, epi, hooks = CASES[case]
    return rows_mx6_decide(n, k, dual, mod=bool(mod), blocks=hooks.get("gemv_rows_blocks", 448), pers=hooks.get("gemv_rows_pers", 192), atomic=atomic)


def test_decision_reaches_exactly_the_enumerated_kernels():
    """Sweeping K over 128 .. 18944, few and many row groups, one and two matrices and the "gemv_rows_blocks" / "gemv_rows_pers" hooks lowered:
    the restated decision names every kernel of ALL_ROWS_MX6 and no other, and every cut covers K with no slice past its end; a modulated
    prologue beyond K = 2048, a SwiGLU row beyond 16 x 8 x 2 loads and a single row beyond 16 x 4 x 4 loads are not covered."""
    got = set()
    for k in range(128, 18944 + 1, 128):
        for n in (32, 48, 1536, 3584, 18944):
            for dual in (0, 1):
                for kw in ({}, {"blocks": 1}, {"blocks": 15}, {"pers": 2}):
                    r = rows_mx6_decide(n, k, dual, **kw)
                    if r is not None:
                        got.add(r[0].split(" ")[0])
                        nw, spw, ksplit = r[1]
                        assert nw * spw * ksplit * 128 >= k > nw * spw * (ksplit - 1) * 128, (n, k, dual, kw, r)
    assert got == set(ALL_ROWS_MX6) and len(ALL_ROWS_MX6) == 10, sorted(got ^ set(ALL_ROWS_MX6))
    assert rows_mx6_decide(32, 2176, 1, mod=True) is None and rows_mx6_decide(32, 2048, 1, mod=True) is not None
    assert rows_mx6_decide(32, 128 * (16 * 8 * 2) + 128, 1) is None and rows_mx6_decide(32, 128 * (16 * 4 * 4) + 128, 0) is None
    # the production shapes (1.5B, 7B; LLM and head)
    assert rows_mx6_decide(1536, 8960, 0)[0] == "gemv_rows_mx6<dual=0,nw=4,ks=3,pers=0> ksplit=6 atomic=0"
    assert rows_mx6_decide(3584, 18944, 0)[0] == "gemv_rows_mx6<dual=0,nw=4,ks=3,pers=0> ksplit=13 atomic=0"
    assert rows_mx6_decide(18944, 3584, 1)[0] == "gemv_rows_mx6<dual=1,nw=8,ks=2,pers=0> ksplit=2 atomic=0"
    assert rows_mx6_decide(8960, 1536, 1)[0] == "gemv_rows_mx6<dual=1,nw=8,ks=2,pers=1> ksplit=1 atomic=0"


def test_cases_reach_every_compiled_instantiation_and_form():
    """The cases' routes (restated decision) are the 10 kernels of the unit: whole rows, the persistent walk over several row groups, the
    ticketed K split and the dual K split, ragged last slices included."""
    routes = {c: route_of_case(c) for c in CASES}
    assert all(r is not None for r in routes.values())
    assert {r[0].split(" ")[0] for r in routes.values()} == set(ALL_ROWS_MX6)
    ragged = [c for c in CASES if routes[c][1][0] * routes[c][1][1] * routes[c][1][2] * 128 > CASES[c][1]]
    assert {"one_load_k384_ragged", "split_k2176_ragged", "split_ks4_k18944", "dual_split_k2176"} <= set(ragged)
    pers = [c for c in CASES if "pers=1" in routes[c][0]]
    assert pers and all(CASES[c][0] // 16 > CASES[c][6]["gemv_rows_pers"] for c in pers), "a persistent block must walk several row groups"
    assert {c for c in CASES if routes[c][1][2] > 1 and CASES[c][2]} == {"dual_split_k2176", "dual_split_ks2_k3584"}
    assert all(32 <= CASES[c][0] <= 80 for c in CASES) and sum(CASES[c][1] > 4608 for c in CASES) == 1, "n in 32..80, one long-K case only"


def test_built_unit_holds_exactly_the_enumerated_kernels(tmp_path):
    """What is compiled is what can launch (reads the symbol table of the object file build() left): the gfx950 code object of
    vv_gemv_rows_mx6.hip holds one gemv_rows_mx6_kernel per entry of ALL_ROWS_MX6 and no other kernel; vv_gemv_rows.hip holds none of them."""
    kernels = built_kernels("vv_gemv_rows_mx6.hip", tmp_path, plain=True)
    assert {k for k, _ in kernels} == {"gemv_rows_mx6_kernel"}, sorted({k for k, _ in kernels})
    got = instantiations_of(kernels, {"gemv_rows_mx6_kernel": _mx6})
    assert got == set(ALL_ROWS_MX6) and len(kernels) == 10, sorted(got ^ set(ALL_ROWS_MX6))
    assert not [k for k, _ in built_kernels("vv_gemv_rows.hip", tmp_path) if "mx6" in k]
    from vibevoice_rocm_amd import build
    assert any(s.endswith("vv_gemv_rows_mx6.hip") for s in build.SRC)


# ---------------------------------------------------------------------------------------------------------------
# vv_linear_route on stand-in addresses
# ---------------------------------------------------------------------------------------------------------------
_A0 = 0x7f0000000000        # stand-in addresses, 256-byte aligned: never followed


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class _tuned:
    DEFAULTS = {"gemv_rows_blocks": 448, "gemv_rows_pers": 192, "gemv_rows_atomic": 1}

    def __init__(self, lb, hooks):
        self.lb, self.hooks = lb, hooks

    def __enter__(self):
        for k, v in self.hooks.items():
            self.lb.vv_tune(k.encode(), v)

    def __exit__(self, *exc):
        for k in self.hooks:
            self.lb.vv_tune(k.encode(), self.DEFAULTS[k])
        return False


def _fake_args(m, n, k, dual=0, pro=0, mod=0, epi=0, in_place=False, flags=_lib.LIN_W_FRAG, wdt=_lib.VV_MXFP6_FRAG, **kw):
    a = _lib.LinArgs()
    MB = 1 << 24
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.flags = _A0, k, m, n, k, wdt, flags
    a.w, a.wscale = _A0 + MB, _A0 + MB + n * k * 3 // 4
    a.out, a.ldo = _A0 + 8 * MB, n
    a.pro, a.eps = pro, 1e-5
    if pro == 1:
        a.norm_w = _A0 + 9 * MB
    if mod:
        a.mod_shift, a.mod_scale, a.ld_mod = _A0 + 10 * MB, _A0 + 11 * MB, k
    if dual:
        a.w2, a.w2scale, a.act = _A0 + 4 * MB, _A0 + 4 * MB + n * k * 3 // 4, _lib.ACT_SWIGLU
    if epi:
        a.gate, a.gate_ld, a.res, a.ldres = _A0 + 12 * MB, n, (a.out if in_place else _A0 + 13 * MB), n
    else:
        a.bias = _A0 + 14 * MB
    for f, v in kw.items():
        setattr(a, f, v)
    return a


def _route(lb, a):
    name = C.create_string_buffer(192)
    rc = lb.vv_linear_route(C.byref(a), name, 192)
    return rc, name.value.decode()


@pytest.mark.parametrize("m", [3, 5, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_route_of_every_case(lib, case, m):
    """K <= 2048: the route query names the instantiation the restated decision predicts.  K > 2048 needs the split-K scratch for the ticketed
    fold, which is device memory: without it the case's own call is refused (VV_E_UNSUPPORTED, no name); the single-matrix cases are asked
    again in place (no prologue, gate and residual with res == out: the atomic split needs no scratch) and name the predicted instantiation
    and cut with atomic=1.  The dual K split's two kernels are the whole-row dual ones, named by the dual cases at K <= 2048."""
    n, k, dual, pro, mod, epi, hooks = CASES[case]
    with _tuned(lib, hooks):
        rc, name = _route(lib, _fake_args(m, n, k, dual, pro, mod, epi))
        if k <= 2048:
            assert (rc, name) == (0, route_of_case(case)[0]), lib.vv_last_error()
            return
        assert (rc, name) == (VV_E_UNSUPPORTED, ""), "a ticketed K split without scratch"
        if not dual:
            rc, name = _route(lib, _fake_args(m, n, k, 0, 0, 0, 1, in_place=True))
            assert (rc, name) == (0, route_of_case(case, atomic=True)[0]) and name.endswith("atomic=1"), lib.vv_last_error()
            with _tuned(lib, {"gemv_rows_atomic": 0}):
                assert _route(lib, _fake_args(m, n, k, 0, 0, 0, 1, in_place=True)) == (VV_E_UNSUPPORTED, "")


def test_every_refusal_is_unsupported_with_an_empty_name(lib):
    """m <= 2, m > 8, the flag missing, n % 16, k % 128, missing scale bytes (of w, of w2), misaligned codes (16) and scale bytes (4), a bf16
    hand-off, VV_LIN_W_MXGEMM, K > 2048 without split-K scratch: VV_E_UNSUPPORTED and no name; the same call without the fault is routed.
    VV_MXFP6 keeps refusing the flag, VV_LIN_W_MXGEMM and 3 rows; 7 stays no weight type."""
    n, k = 64, 1024
    ok = lambda **kw: _fake_args(kw.pop("m", 4), kw.pop("n", n), kw.pop("k", k), **kw)      # noqa: E731
    base = ok()
    p, q = base.w, base.wscale
    dual = dict(dual=1)
    refused = {"m=1": ok(m=1), "m=2": ok(m=2), "m=9": ok(m=9), "m=16": ok(m=16), "no flag": ok(flags=0), "n%16": ok(n=56), "n<16": ok(n=8),
               "k%128": ok(k=k - 64), "k%128 (32)": ok(k=k + 32), "no wscale": ok(wscale=None), "no w2scale": ok(**dual, w2scale=None),
               "w+8": ok(w=p + 8), "w2+8": ok(**dual, w2=p + 8), "wscale+2": ok(wscale=q + 2), "w2scale+1": ok(**dual, w2scale=q + 1),
               "x bf16": ok(flags=_lib.LIN_W_FRAG | _lib.LIN_X_BF16), "out bf16": ok(flags=_lib.LIN_W_FRAG | _lib.LIN_OUT_BF16),
               "mxgemm": ok(flags=_lib.LIN_W_FRAG | _lib.LIN_W_MXGEMM), "mxgemm, bf16 x": ok(m=16, flags=_lib.LIN_W_MXGEMM | _lib.LIN_X_BF16),
               "k=4096 without scratch": ok(k=4096),
               "VV_MXFP6 + flag": ok(wdt=_lib.VV_MXFP6), "VV_MXFP6, 3 rows": ok(m=3, flags=0, wdt=_lib.VV_MXFP6),
               "VV_MXFP6 + mxgemm": ok(m=16, flags=_lib.LIN_W_MXGEMM | _lib.LIN_X_BF16, wdt=_lib.VV_MXFP6)}
    for what, a in refused.items():
        rc, name = _route(lib, a)
        assert (rc, name) == (VV_E_UNSUPPORTED, ""), (what, rc, name, lib.vv_last_error())
    rc, name = _route(lib, ok(wdt=7))
    assert rc == -1 and name == "", "7 is no weight type (VV_E_ARG)"
    for a in (ok(), ok(m=3), ok(m=8, **dual), ok(k=2048), ok(k=4096, epi=1, in_place=True)):
        rc, name = _route(lib, a)
        assert rc == 0 and name.startswith("gemv_rows_mx6<"), lib.vv_last_error()
    rc, name = _route(lib, ok(m=2, flags=0, wdt=_lib.VV_MXFP6, wscale=q))
    assert rc == 0 and name.startswith("gemv_mx6<m=2"), "the streaming GEMV's calls are taken as before"


# ---------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------
def _random_mx6(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 64, (n, k), generator=g).to(torch.uint8), torch.randint(2, 253, (n, k // 32), generator=g).to(torch.uint8)


@pytest.mark.parametrize("n,k", [(16, 128), (32, 256), (48, 384)])
def test_frag_major_mxfp6_matches_the_layout_sentence(n, k):
    """One and several row groups and 128-wide steps.  include/vv_hip.h (VV_MXFP6_FRAG): lane 16 c + n of step J of row group g owns block
    4 J + c of row 16 g + n; code i of the block sits in bits 6 i .. 6 i + 5 of its 24-byte string, whose bytes 0..15 lie in plane A at
    ((g K/128 + J) 64 + lane) 16 and bytes 16..23 in plane B at N K / 2 + ((g K/128 + J) 64 + lane) 8; the block's scale byte is byte c of the
    dword at N K 3/4 + ((g K/128 + J) 16 + n) 4.  Every (row, k) is looked up there."""
    codes, scales = _random_mx6(n, k, 7 + n)
    f = DeviceWeights.frag_major_mxfp6(codes, scales)
    assert f.dtype == torch.uint8 and f.dim() == 1 and f.numel() == n * k * 25 // 32 and (n * k // 2) % 1024 == 0 and (n * k * 3 // 4) % 512 == 0
    by = f.tolist()
    kj = k // 128
    for row in range(n):
        g, r = divmod(row, 16)
        for col in range(k):
            J, c, i = col // 128, (col % 128) // 32, col % 32
            slot = (g * kj + J) * 64 + 16 * c + r
            got = 0
            for j in range(6):
                bit = 6 * i + j
                byte = by[slot * 16 + bit // 8] if bit < 128 else by[n * k // 2 + slot * 8 + (bit - 128) // 8]
                got |= ((byte >> (bit % 8)) & 1) << j
            assert got == int(codes[row, col]), (row, col)
            assert by[n * k * 3 // 4 + ((g * kj + J) * 16 + r) * 4 + c] == int(scales[row, col // 32]), (row, col)


@pytest.mark.parametrize("n,k", [(16, 128), (32, 256), (48, 384), (64, 1152)])
def test_unfrag_mxfp6_round_trip(n, k):
    codes, scales = _random_mx6(n, k, n + k)
    c2, s2 = DeviceWeights.unfrag_mxfp6(DeviceWeights.frag_major_mxfp6(codes, scales), n, k)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


@pytest.mark.parametrize("n,k", [(24, 128), (17, 256), (32, 64), (32, 192), (16, 96)])
def test_frag_major_mxfp6_refuses_other_shapes(n, k):
    codes, scales = _random_mx6(n, k, 1)
    assert DeviceWeights.frag_major_mxfp6(codes, scales) is None


# ---------------------------------------------------------------------------------------------------------------
# the keyword, the descriptor bit and the fragment copies (no GPU: DeviceWeights on the CPU at `tiny`)
# ---------------------------------------------------------------------------------------------------------------
def test_header_and_lib_agree(lib):
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    assert re.search(r"enum \{ VV_MXFP6_FRAG = 8 \};", hdr) and re.search(r"enum \{ VV_WQ_FRAG6 = 0x1000 \};", hdr)
    assert (_lib.VV_MXFP6_FRAG, _lib.VV_WQ_FRAG6, _lib.VV_MXFP6, _lib.VV_WQ_MXFP6, _lib.VV_WQ_FRAG4) == (8, 0x1000, 6, 0x800, 0x400)
    assert "Value 7 is no weight type" in hdr
    assert "Plane A [N / 16][K / 128][64 lanes][16 B]" in hdr and "Plane B [N / 16][K / 128][64 lanes][8 B]" in hdr
    assert "gemv_rows_mx6<dual=0,nw=4,ks=3,pers=0> ksplit=6 atomic=0" in hdr
    assert lib.vv_abi_version() == 6, "no struct changed: the ABI version stays"


@pytest.mark.parametrize("quant", [None, "fp8", "nf4", "mxfp4"])
def test_keyword_needs_mxfp6(tiny_cfg, quant):
    """mxfp6_row_batch=True with another weight_quant raises ValueError before a weight or a device is touched (an empty state dict is enough)"""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    with pytest.raises(ValueError, match="mxfp6_row_batch"):
        M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=quant, mxfp6_row_batch=True)
    with pytest.raises(ValueError, match="mxfp6_row_batch"):
        M.from_synthetic(tiny_cfg, 1, numpy_weights=True, weight_quant=quant, mxfp6_row_batch=True)
    with pytest.raises(ValueError, match="mxfp6_row_batch"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant=quant, mxfp6_row_batch=True)


def test_keyword_refuses_wide_batches_conv_rows_and_large_hidden(tiny_cfg):
    """row_batch_width=8 (the 16-row GEMV is bf16-only), batched_conv_rows=True (bf16 without companions only) and an LLM hidden size beyond
    4096 - the SwiGLU pair would need a three-way K split (2 loads x 8 waves x 128 per slice), more than the row-batched step's partials
    workspace holds - raise ValueError before any device work; 4096 and the keyword off are not refused on the last ground.  The sibling
    keywords keep naming themselves on an mxfp6 model."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    kw = dict(device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", mxfp6_row_batch=True)
    with pytest.raises(ValueError, match="row_batch_width=8"):
        M(tiny_cfg, {}, row_batch_width=8, **kw)
    with pytest.raises(ValueError, match="batched_conv_rows=True"):
        M(tiny_cfg, {}, batched_conv_rows=True, **kw)
    big = dataclasses.replace(tiny_cfg, hidden=4224)
    with pytest.raises(ValueError, match="mxfp6_row_batch=True serves LLM hidden sizes up to 4096"):
        M(big, {}, **kw)
    with pytest.raises(ValueError, match="hidden sizes up to 4096"):
        DeviceWeights(big, {}, "cpu", torch.bfloat16, quant="mxfp6", mxfp6_row_batch=True)
    for hidden, k2 in ((4096, dict(mxfp6_row_batch=True)), (4224, {})):
        with pytest.raises(Exception) as ei:                # no weights given: the construction fails further on, not on the hidden size
            DeviceWeights(dataclasses.replace(tiny_cfg, hidden=hidden), {}, "cpu", torch.bfloat16, quant="mxfp6", **k2)
        assert "hidden sizes up to" not in str(ei.value)
    for k2, word in ((dict(mxfp4_row_batch=True), "mxfp4_row_batch"), (dict(mxfp4_lean=True), "mxfp4_lean")):
        with pytest.raises(ValueError, match=word):
            M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", **k2)


def test_row_batch_ok_and_the_session_check():
    """row_batch_ok admits "mxfp6" with the keyword alone; the model's row-batch and session checks read it (an mxfp6 model without the keyword:
    batches on the lanes, open_session refused with weight_quant='mxfp6' in the text)"""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    from vibevoice_rocm_amd.rowbatch import row_batch_ok
    assert row_batch_ok(None) and row_batch_ok("fp8") and not row_batch_ok("nf4")
    assert not row_batch_ok("mxfp6") and row_batch_ok("mxfp6", mxfp6_row_batch=True) and not row_batch_ok("mxfp6", mxfp4_row_batch=True)
    assert not row_batch_ok("mxfp4") and row_batch_ok("mxfp4", mxfp4_row_batch=True) and not row_batch_ok("mxfp4", mxfp6_row_batch=True)

    def shell(**kw):          # the checks read attributes only: no device, no weights
        m = object.__new__(M)
        m.__dict__.update(dict(weight_quant="mxfp6", mxfp4_row_batch=False, mxfp6_row_batch=False, dtype=torch.bfloat16, kv_cache_dtype=None,
                               _use_graphs=True, _session=None), **kw)
        return m

    assert not shell()._rows_quant_ok() and shell(mxfp6_row_batch=True)._rows_quant_ok()
    with pytest.raises(ValueError, match="weight_quant='mxfp6'"):
        shell().open_session(tokenizer=object(), slots=2, max_context=64)


def test_descriptor_bit_and_fragment_copies(tiny_cfg, tiny_weights):
    """The bit rides on the LLM's and the head's descriptors only with the keyword.  With it ensure_frag builds the VV_MXFP6_FRAG form of every
    companion whose shape fits (at `tiny`: the LLM's down projection, [64, 128]) - codes and scale bytes equal to the companion's own, 0.78125
    bytes per weight, counted by nbytes() - and leaves every other f_* NULL (never a bf16 copy); built once for the weights and their forks.
    Without it nothing differs from before: no bit, and bf16 copies where the shapes allow."""
    cfg = tiny_cfg
    w = DeviceWeights(cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp6", mxfp6_row_batch=True)
    w0 = DeviceWeights(cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp6")
    both = _lib.VV_BF16 | _lib.VV_WQ_MXFP6
    assert (w.llm.wdt, w.head.wdt) == (both | _lib.VV_WQ_FRAG6,) * 2 and (w0.llm.wdt, w0.head.wdt) == (both, both)
    assert w.dec.wdt == w.sem.wdt == both and w.mxfp6_row_batch and not w0.mxfp6_row_batch and not w.mxfp4_row_batch
    assert not w._frag_state["tensors"] and not w0._frag_state["tensors"], "fragment copies are built on first use only"
    before = w.nbytes()
    w.ensure_frag()
    by_ptr = {t.data_ptr(): t for t in w._frag_state["tensors"]}
    keep = {t.data_ptr(): t for t in w._keep if isinstance(t, torch.Tensor)}
    n_copied = 0
    for l in range(cfg.layers):
        lay = w.llm.layer[l]
        for nm, (n, k) in {"qkv": ((cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, cfg.hidden), "o": (cfg.hidden, cfg.heads * cfg.head_dim),
                           "gate": (cfg.inter, cfg.hidden), "up": (cfg.inter, cfg.hidden), "down": (cfg.hidden, cfg.inter)}.items():
            p, q = getattr(lay, "f_" + nm), getattr(lay, "q_" + nm)
            if n % 16 or k % 128:
                assert not p, f"layer {l} f_{nm}: a copy of a shape the form cannot take"
                continue
            f = by_ptr[p]
            assert f.dtype == torch.uint8 and f.numel() == n * k * 25 // 32 and p % 16 == 0
            want = unpack_mxfp6(keep[q.q], keep[q.scale], n, k)
            got = DeviceWeights.unfrag_mxfp6(f, n, k)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            n_copied += n * k
    assert n_copied == cfg.layers * cfg.hidden * cfg.inter > 0
    for l in range(cfg.head_layers):
        assert not any(getattr(w.head.layer[l], "f_" + nm) for nm in ("gate", "up", "down"))      # K = 64 / 192: no copy, and no bf16 copy either
    st = w._frag_state
    assert st["mxfp6_weights"] == n_copied and st["mxfp6_bytes"] == n_copied * 25 // 32 == w.nbytes() - before and st["mxfp4_bytes"] == 0
    n_t = len(st["tensors"])
    w.fork().ensure_frag()
    w.ensure_frag()
    assert len(st["tensors"]) == n_t, "built once per weight set and its forks"
    w0.ensure_frag()
    assert w0._frag_state["tensors"] and all(t.dtype == torch.bfloat16 for t in w0._frag_state["tensors"]) and w0._frag_state["mxfp6_bytes"] == 0
