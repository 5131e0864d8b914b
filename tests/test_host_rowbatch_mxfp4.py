"""CPU tests of MXFP4 on the row-batched decode path (weight_quant="mxfp4", mxfp4_row_batch=True; csrc/vv_gemv_rows.hip):
the fragment-major VV_MXFP4_FRAG packing against the header's index formula, its inverse, the shapes it refuses, the opt-in keyword and the
descriptor bit, the fragment copies ensure_frag builds (on the CPU, at `tiny`), the decision's rules restated (shared with
tests/test_hip_rowbatch_mxfp4.py) and the MXFP4 kernel set of the built unit."""
import os
import re

import pytest
import torch

from test_hip_mfma_gemm import built_kernels, instantiations_of
from vibevoice_rocm_amd import _lib
from vibevoice_rocm_amd.weights import DeviceWeights, unpack_mxfp4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------
# the decision's rules, restated (vv_gemv_rows.hip: vv_gemv_rows_decide on VV_MXFP4_FRAG weights, and the bf16 form's K cut)
# ---------------------------------------------------------------------------------------------------------------
MAXSPLIT = 16


def _mxr(dual, nw, ks, pers):
    return f"gemv_rows_mx<dual={dual},nw={nw},ks={ks},pers={pers}>"


# every MXFP4 kernel of the unit (gemv_rows_kernel<dual, nw, ks, pers, 2>): whole rows (8 waves, 1 or 2 loads of 128 k per wave; SwiGLU also persistent), the SwiGLU K split (the same two
# kernels), the single-matrix K split (4 waves, 1..4 loads)
ALL_ROWS_MX = [_mxr(0, 8, 1, 0), _mxr(0, 8, 2, 0), _mxr(1, 8, 1, 0), _mxr(1, 8, 2, 0), _mxr(1, 8, 1, 1), _mxr(1, 8, 2, 1),
               _mxr(0, 4, 1, 0), _mxr(0, 4, 2, 0), _mxr(0, 4, 3, 0), _mxr(0, 4, 4, 0)]


def _split(steps, n_groups, nw, kscap, ksmax, few, blocks):
    """(ksplit, loads per wave) of a K split over `steps` weight loads, or None: the first split whose waves take <= kscap loads and that gives
    `blocks` workgroups (or leaves <= `few` loads per wave), else the first with <= ksmax loads; slices that would start past the end are dropped"""
    pick = next(((sp, -(-steps // (sp * nw))) for sp in range(2, MAXSPLIT + 1)
                 if -(-steps // (sp * nw)) <= kscap and (n_groups * sp >= blocks or -(-steps // (sp * nw)) <= few)), None)
    if pick is None:
        pick = next(((sp, -(-steps // (sp * nw))) for sp in range(2, MAXSPLIT + 1) if -(-steps // (sp * nw)) <= ksmax), None)
    if pick is None:
        return None
    ksplit, spw = pick
    while ksplit > 1 and (ksplit - 1) * nw * spw >= steps:
        ksplit -= 1
    return ksplit, spw


def rows_mx_decide(n, k, dual, mod=False, blocks=448, pers=192, atomic=False):
    """(route name as vv_linear_route prints it, K cut (waves, 32-wide k steps per wave, K slices)) of an aligned 3..8-row VV_MXFP4_FRAG call with
    split-K scratch, or None (not covered)"""
    if n % 16 or k % 128:
        return None
    steps, n_groups = k // 128, n // 16
    if steps <= 16:
        spw = (steps + 7) // 8
        p = int(bool(dual) and n_groups > pers)
        return f"{_mxr(int(dual), 8, spw, p)} ksplit=1 atomic=0", (8, 4 * spw, 1)
    if mod:
        return None
    nw = 8 if dual else 4
    cut = _split(steps, n_groups, nw, 2 if dual else 3, 2 if dual else 4, 1, blocks)
    if cut is None:
        return None
    ksplit, spw = cut
    return f"{_mxr(int(dual), nw, spw, 0)} ksplit={ksplit} atomic={int(atomic and not dual)}", (nw, 4 * spw, ksplit)


def rows_bf16_cut(n, k, dual, blocks=448):
    """the K cut (waves, 32-wide k steps per wave, K slices) of the bf16 fragment-major form of the same call (vv_gemv_rows_decide)"""
    steps, n_groups = k // 32, n // 16
    if steps <= 64:
        return 8, (steps + 7) // 8, 1
    nw = 8 if dual else 4
    ksplit, spw = _split(steps, n_groups, nw, 8 if dual else 9, 8 if dual else 12, 3, blocks)
    return nw, spw, ksplit


def test_decision_reaches_exactly_the_enumerated_kernels():
    """Sweeping K over 128 .. 18944, few and many row groups, one and two matrices, with and without the adaLN prologue and with the
    "gemv_rows_blocks" / "gemv_rows_pers" hooks lowered: the restated decision names every kernel of ALL_ROWS_MX and no other; a modulated
    prologue beyond K = 2048 and a SwiGLU row beyond 2 x 8 x 2 x 16 loads are not covered."""
    got = set()
    for k in range(128, 18944 + 1, 128):
        for n in (32, 48, 1536, 3584, 18944):
            for dual in (0, 1):
                for kw in ({}, {"blocks": 1}, {"blocks": 15}, {"pers": 2}):
                    r = rows_mx_decide(n, k, dual, **kw)
                    if r is not None:
                        got.add(r[0].split(" ")[0])
                        nw, spa, ksplit = r[1]
                        assert nw * spa * ksplit * 32 >= k > nw * spa * (ksplit - 1) * 32, (n, k, dual, kw, r)
    assert got == set(ALL_ROWS_MX) and len(ALL_ROWS_MX) == 10, sorted(got ^ set(ALL_ROWS_MX))
    assert rows_mx_decide(32, 2176, 1, mod=True) is None and rows_mx_decide(32, 2048, 1, mod=True) is not None
    assert rows_mx_decide(32, 128 * (16 * 8 * 2) + 128, 1) is None and rows_mx_decide(32, 128 * (16 * 4 * 4) + 128, 0) is None
    # the production shapes (1.5B, 7B; LLM and head): name and cut
    assert rows_mx_decide(1536, 8960, 0)[0] == "gemv_rows_mx<dual=0,nw=4,ks=3,pers=0> ksplit=6 atomic=0"
    assert rows_mx_decide(1536, 4608, 0)[0] == "gemv_rows_mx<dual=0,nw=4,ks=2,pers=0> ksplit=5 atomic=0"
    assert rows_mx_decide(3584, 18944, 0)[0] == "gemv_rows_mx<dual=0,nw=4,ks=3,pers=0> ksplit=13 atomic=0"
    assert rows_mx_decide(18944, 3584, 1)[0] == "gemv_rows_mx<dual=1,nw=8,ks=2,pers=0> ksplit=2 atomic=0"
    assert rows_mx_decide(8960, 1536, 1)[0] == "gemv_rows_mx<dual=1,nw=8,ks=2,pers=1> ksplit=1 atomic=0"


def test_built_unit_holds_exactly_the_enumerated_kernels(tmp_path):
    """What is compiled is what can launch (reads the symbol table of the object file build() left): the gfx950 code object of
    vv_gemv_rows.hip holds one gemv_rows_kernel of weight format 2 (MXFP4) per entry of ALL_ROWS_MX and no other.  The unit's kernels of
    formats 0 and 1 (bf16, fp8) are the 22 of tests/test_hip_gemv.py's ALL_INSTANTIATIONS, held to exactly that set by its
    test_built_library_holds_exactly_the_enumerated_kernels: between the two lists every gemv_rows_kernel of the binary is claimed by one of
    them and nothing is left over - 32 kernels, no other format."""
    kernels = [args for k, args in built_kernels("vv_gemv_rows.hip", tmp_path) if k == "gemv_rows_kernel"]
    assert sorted({args[4] for args in kernels}) == ["0", "1", "2"] and len(kernels) == 22 + len(ALL_ROWS_MX), kernels
    got = instantiations_of([("mx", args[:4]) for args in kernels if args[4] == "2"], {"mx": _mxr})
    assert got == set(ALL_ROWS_MX), sorted(got ^ set(ALL_ROWS_MX))


# ---------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------
def _random_mx(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 16, (n, k), generator=g).to(torch.uint8), torch.randint(2, 253, (n, k // 32), generator=g).to(torch.uint8)


def test_frag_major_mxfp4_matches_the_index_formula():
    """[32, 256]: two row groups, two 128-wide steps.  Every code and every scale byte sits where include/vv_hip.h (VV_MXFP4_FRAG) says."""
    n, k = 32, 256
    codes, scales = _random_mx(n, k, 7)
    f = DeviceWeights.frag_major_mxfp4(codes, scales)
    assert f.dtype == torch.uint8 and f.dim() == 1 and f.numel() == n * k // 2 + n * k // 32 and (n * k // 2) % 1024 == 0
    dw = f[: n * k // 2].view(-1, 4).int()
    dw = dw[:, 0] | (dw[:, 1] << 8) | (dw[:, 2] << 16) | (dw[:, 3] << 24)
    sb = f[n * k // 2:]
    kj = k // 128
    for row in range(n):
        g, r = divmod(row, 16)
        for col in range(k):
            J, h, c, i = col // 128, (col % 128) // 32, (col % 32) // 8, col % 8
            lane = 16 * c + r
            assert (int(dw[((g * kj + J) * 64 + lane) * 4 + h]) >> (4 * i)) & 15 == int(codes[row, col]), (row, col)
            assert int(sb[((g * kj + J) * 16 + r) * 4 + h]) == int(scales[row, col // 32]), (row, col)


@pytest.mark.parametrize("n,k", [(16, 128), (32, 256), (48, 384), (64, 1152)])
def test_unfrag_mxfp4_round_trip(n, k):
    codes, scales = _random_mx(n, k, n + k)
    c2, s2 = DeviceWeights.unfrag_mxfp4(DeviceWeights.frag_major_mxfp4(codes, scales), n, k)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)


@pytest.mark.parametrize("n,k", [(24, 128), (17, 256), (32, 64), (32, 192), (16, 96)])
def test_frag_major_mxfp4_refuses_other_shapes(n, k):
    codes, scales = _random_mx(n, k, 1)
    assert DeviceWeights.frag_major_mxfp4(codes, scales) is None


# ---------------------------------------------------------------------------------------------------------------
# the keyword, the descriptor bit and the fragment copies (no GPU: DeviceWeights on the CPU at `tiny`)
# ---------------------------------------------------------------------------------------------------------------
def test_header_and_lib_agree():
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    assert re.search(r"enum \{ VV_MXFP4_FRAG = 5 \};", hdr) and re.search(r"enum \{ VV_WQ_FRAG4 = 0x400 \};", hdr)
    assert (_lib.VV_MXFP4_FRAG, _lib.VV_WQ_FRAG4, _lib.VV_MXFP4, _lib.VV_WQ_MXFP4) == (5, 0x400, 4, 0x200)
    assert "[N / 16][K / 128][64 lanes][16 B]" in hdr and "[N / 16][K / 128][16 rows][4 B]" in hdr


@pytest.mark.parametrize("quant", [None, "fp8", "nf4"])
def test_keyword_needs_mxfp4(tiny_cfg, quant):
    """mxfp4_row_batch=True with another weight_quant raises ValueError: the model's constructor and the engine's weights layer before a weight
    or a device is touched (an empty state dict is enough), from_synthetic through the constructor, once it has synthesised its state dict."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    with pytest.raises(ValueError, match="mxfp4_row_batch"):
        M(tiny_cfg, {}, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant=quant, mxfp4_row_batch=True)
    with pytest.raises(ValueError, match="mxfp4_row_batch"):
        M.from_synthetic(tiny_cfg, 1, numpy_weights=True, weight_quant=quant, mxfp4_row_batch=True)
    with pytest.raises(ValueError, match="mxfp4_row_batch"):
        DeviceWeights(tiny_cfg, {}, "cpu", torch.bfloat16, quant=quant, mxfp4_row_batch=True)


def test_keyword_refuses_a_hidden_size_beyond_the_two_way_split(tiny_cfg):
    """LLM hidden > 4096: the SwiGLU pair would need a three-way K split (2 loads x 8 waves x 128 per slice), which the row-batched step's
    partials workspace has no room for - the call would quietly run on the bf16 matrices.  The opt-in refuses such a config instead; 4096 and
    the keyword off are not refused on this ground."""
    import dataclasses
    with pytest.raises(ValueError, match="hidden sizes up to 4096"):
        DeviceWeights(dataclasses.replace(tiny_cfg, hidden=4224), {}, "cpu", torch.bfloat16, quant="mxfp4", mxfp4_row_batch=True)
    for hidden, kw in ((4096, dict(mxfp4_row_batch=True)), (4224, {})):
        with pytest.raises(Exception) as ei:                # no weights given: the construction fails further on, not on the hidden size
            DeviceWeights(dataclasses.replace(tiny_cfg, hidden=hidden), {}, "cpu", torch.bfloat16, quant="mxfp4", **kw)
        assert "hidden sizes up to" not in str(ei.value)


def test_descriptor_bit_and_fragment_copies(tiny_cfg, tiny_weights):
    """The bit rides on the LLM's and the head's descriptors only with the keyword.  With it ensure_frag builds the VV_MXFP4_FRAG form of every
    companion whose shape fits (at `tiny`: the LLM's down projection, [64, 128]) - codes and scale bytes equal to the companion's own, 0.53125
    bytes per weight, counted by nbytes() - and leaves every other f_* NULL (never a bf16 copy); without it nothing differs from the parent:
    no bit, and bf16 copies where the shapes allow."""
    cfg = tiny_cfg
    w = DeviceWeights(cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp4", mxfp4_row_batch=True)
    w0 = DeviceWeights(cfg, tiny_weights, "cpu", torch.bfloat16, quant="mxfp4")
    both = _lib.VV_BF16 | _lib.VV_WQ_MXFP4
    assert (w.llm.wdt, w.head.wdt) == (both | _lib.VV_WQ_FRAG4,) * 2 and (w0.llm.wdt, w0.head.wdt) == (both, both)
    assert w.dec.wdt == w.sem.wdt == both and w.mxfp4_row_batch and not w0.mxfp4_row_batch
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
            assert f.dtype == torch.uint8 and f.numel() == n * k // 2 + n * k // 32
            want = unpack_mxfp4(keep[q.q], keep[q.scale], n, k)
            got = DeviceWeights.unfrag_mxfp4(f, n, k)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            n_copied += n * k
    assert n_copied == cfg.layers * cfg.hidden * cfg.inter > 0
    for l in range(cfg.head_layers):
        assert not any(getattr(w.head.layer[l], "f_" + nm) for nm in ("gate", "up", "down"))      # K = 64 / 192: no copy, and no bf16 copy either
    st = w._frag_state
    assert st["mxfp4_weights"] == n_copied and st["mxfp4_bytes"] == n_copied * 17 // 32 == w.nbytes() - before
    n_t = len(st["tensors"])
    w.fork().ensure_frag()
    w.ensure_frag()
    assert len(st["tensors"]) == n_t, "built once per weight set and its forks"
    w0.ensure_frag()
    assert w0._frag_state["tensors"] and all(t.dtype == torch.bfloat16 for t in w0._frag_state["tensors"]) and w0._frag_state["mxfp4_bytes"] == 0
