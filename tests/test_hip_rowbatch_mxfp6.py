"""GPU parity of MXFP6 on the row-batched decode path (weight_quant="mxfp6", mxfp6_row_batch=True; csrc/vv_gemv_rows_mx6.hip).

1. the kernel: decode read back exactly (every e2m3 code at every position of a block, scale bytes 2 / 127 / 252: this is what catches a wrong k
   permutation), then vv_linear on VV_MXFP6_FRAG against vv_linear on the bf16 fragment-major copy of the effective matrix (rel RMS < 1e-6: the
   same products in another summation order, never bit for bit), against fp64 torch per element (< 2e-5) and in place with the atomic split
   (< 2e-5) - the bars tests/test_hip_rowbatch_mxfp4.py uses for the same comparisons.  m in {3, 5, 8}; the cases of
   tests/test_host_rowbatch_mxfp6.py (every compiled instantiation in every form); every case twice into separate outputs, bit-identical
   (tickets left ready), NaN gaps and guard rows intact, inputs unchanged.
2. refusals: VV_E_UNSUPPORTED from vv_linear itself, nothing written.
3. the engine at `mid`: the 8-row decode step against the batch-2 MXFP6 step, the batched head sampler against the single one, generate() on 3
   and 4 dialogues row batch against lanes and against the oracle on the effective weights, what the row batch streams (profiler record), the
   fragment copies built once.
4. a two-slot session on that model.  5. the 7B widths (2 layers), GPU against GPU.
Measured errors go into the parity record (conftest.rel_rms `what=`)."""
import ctypes as C
import dataclasses
import gc

import pytest
import torch

from conftest import rel_rms
from test_host_rowbatch_mxfp6 import ALL_ROWS_MX6, CASES, route_of_case

pytestmark = pytest.mark.gpu

VV_E_UNSUPPORTED = -3
N_STEPS = 20
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    lb = L.load()
    L.check(lb.vv_init(), "vv_init")
    return lb


class _tuned:
    """vv_tune hooks for one case (the rows unit's one tune state), restored to the defaults on exit"""
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


def _values(device):
    from vibevoice_rocm_amd.weights import MXFP6_VALUES
    return torch.tensor(MXFP6_VALUES + tuple(-v for v in MXFP6_VALUES), dtype=torch.float64, device=device)


def _effective(codes, scales):
    """value(code) * 2^(e - 127) in fp64, [n, k]"""
    return _values(codes.device)[codes.long()] * torch.exp2(scales.double() - 127).repeat_interleave(32, dim=1)


# ---------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------
def test_decode_is_exact(lib):
    """Every weight of a [32, 256] matrix (two row groups, two 128-wide loads, 256 blocks) read back through the kernel with one-hot activation
    rows (8 columns per launch).  Code (r + 32 (b & 1) + 5 i) mod 64 at element i of block b of row r: all 64 codes at every one of the 32
    positions.  Scale bytes 2, 127 and 252 (and 64, 200, 120, 134) over all rows and blocks; under byte 2 the codes below 4/8 are fp32
    subnormals.  Each output must be value(code) * 2^(e - 127) bit for bit (a zero weight reads +0).  Pins the bit order inside a block, the
    plane split, the block-to-lane assignment, the k permutation of the four MFMAs of a load and the scale byte's place."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.weights import DeviceWeights
    n, k = 32, 256
    r, c = torch.arange(n)[:, None], torch.arange(k)[None, :]
    codes = ((r + 32 * ((c // 32) & 1) + 5 * (c % 32)) % 64).to(torch.uint8).cuda()
    for i in range(32):
        assert len(set(codes[:, i::32].flatten().tolist())) == 64, f"position {i} does not see every code"
    scales = torch.tensor([2, 64, 127, 200, 252, 120, 134, 127], dtype=torch.uint8)[(torch.arange(n)[:, None] + torch.arange(k // 32)[None, :] * 3) % 8].cuda()
    assert {2, 127, 252} <= set(scales.flatten().tolist())
    f = DeviceWeights.frag_major_mxfp6(codes, scales)
    want = _effective(codes, scales).float()
    assert torch.equal(want.double(), _effective(codes, scales)), "value(code) * 2^(e - 127) must be exact in fp32"
    want = torch.where(want == 0, torch.zeros_like(want), want)
    got = torch.empty(k, n, device="cuda")
    x = torch.zeros(k // 8, 8, k, device="cuda")
    for j in range(k // 8):
        x[j, torch.arange(8), 8 * j + torch.arange(8)] = 1.0
    for j in range(k // 8):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.flags = x[j].data_ptr(), k, 8, n, k, L.VV_MXFP6_FRAG, L.LIN_W_FRAG
        a.w, a.wscale = f.data_ptr(), f.data_ptr() + n * k * 3 // 4
        a.out, a.ldo = got[8 * j:].data_ptr(), n
        L.check(lib.vv_linear(C.byref(a), torch.cuda.current_stream().cuda_stream), "vv_linear")
    torch.cuda.synchronize()
    bad = (got.t().contiguous().view(torch.int32) != want.view(torch.int32))
    assert not bad.any(), f"{int(bad.sum())} weights decode wrong, first at {bad.nonzero()[0].tolist()}: " \
                          f"got {got.t()[tuple(bad.nonzero()[0].tolist())].item()!r} want {want[tuple(bad.nonzero()[0].tolist())].item()!r}"


def _planted(n, k, seed, x_free_block):
    """MXFP6 codes [n, k] / scale bytes [n, k / 32] of a random matrix with all 64 codes (-0 = code 32 included) planted in every row and scale
    bytes 2, 127 and 252 planted in blocks 1, 2 and `x_free_block` of rows 1, 17, ...; returns (codes, scales, effective matrix bf16 - exact)"""
    from vibevoice_rocm_amd.weights import quantize_mxfp6
    g = torch.Generator(device="cuda").manual_seed(seed)
    codes, scales, _ = quantize_mxfp6((torch.randn(n, k, device="cuda", generator=g) / k ** 0.5).bfloat16())
    rows = torch.arange(n, device="cuda")
    for c in range(64):
        codes[rows, (rows * 5 + c * 7 + 3) % 64] = c                 # 64 distinct columns of blocks 0 and 1 (7 is a unit mod 64), shifted per row
    nb = k // 32
    scales[1::16, 1 % nb] = 2
    scales[1::16, 2 % nb] = 127
    scales[1::16, x_free_block] = 252
    eff = _effective(codes, scales)
    eff16 = eff.bfloat16()
    assert torch.equal(eff16.double(), eff), "value(code) * 2^(e - 127) must be exact in bf16"
    return codes.contiguous(), scales.contiguous(), eff16


def test_cases_reach_every_compiled_instantiation():
    """CPU assertion: the cases' routes (restated decision, tests/test_host_rowbatch_mxfp6.py) are exactly the 10 kernels of the unit"""
    assert {route_of_case(c)[0].split(" ")[0] for c in CASES} == set(ALL_ROWS_MX6)


@pytest.mark.parametrize("m_rows", [3, 5, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_gemv_mxfp6_frag(lib, case, m_rows):
    """vv_linear on VV_MXFP6_FRAG (ticketed split, gemv_rows_atomic = 0) twice into two NaN-framed outputs: bit-identical, gaps and guard rows
    intact, inputs unchanged.  Against vv_linear on the bf16 fragment-major copy of the effective matrix: rel RMS < 1e-6 (the same products,
    another summation order).  Against fp64 torch: < 2e-5; the K-split cases with a linear in-place epilogue also in the atomic form: < 2e-5.
    The route is the restated decision's.  Scale byte 252 sits in the last block of rows 1, 17, ...: its activations are bf16-exact multiples of
    2^-125 (no prologue) or zero (a prologue would rescale them), so every product stays finite."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.weights import DeviceWeights
    n, k, dual, pro, mod, epi, hooks = CASES[case]
    m = m_rows
    want_route = route_of_case(case)[0]
    L.check(lib.vv_tune(b"gemv_rows_scratch", 1), "scratch")
    try:
        with _tuned(lib, {**hooks, "gemv_rows_atomic": 0}):
            torch.manual_seed(m * 1000 + n + k)
            xb = (k // 32) - 1
            x = torch.randn(m, k, device="cuda") * 1.5
            x[:, 32 * xb:] = 0.0 if pro else (1 + torch.randint(0, 128, (m, 32), device="cuda") / 128.0) * torch.where(torch.rand(m, 32, device="cuda") < 0.5, -1.0, 1.0) * 2.0 ** -125
            q1, s1, e1 = _planted(n, k, n + k, xb)
            q2, s2, e2 = _planted(n, k, n + k + 1, xb) if dual else (None, None, None)
            nw = torch.rand(k, device="cuda") + 0.5
            sh, sc = torch.randn(m, k, device="cuda") * 0.2, torch.randn(m, k, device="cuda") * 0.2
            sh[:, 32 * xb:] = 0.0
            gate, res, b = torch.randn(m, n, device="cuda"), torch.randn(m, n, device="cuda"), torch.randn(n, device="cuda")
            fx = {1: DeviceWeights.frag_major_mxfp6(q1, s1), 2: DeviceWeights.frag_major_mxfp6(q2, s2) if dual else None}
            fb = {1: DeviceWeights.frag_major(e1), 2: DeviceWeights.frag_major(e2) if dual else None}
            assert fx[1] is not None and fb[1] is not None and fx[1].data_ptr() % 16 == 0
            inputs = [t for t in (x, nw, sh, sc, gate, res, b, fx[1], fx[2]) if t is not None]
            kept = [t.clone() for t in inputs]
            ldo = n + 8                                   # a gap of 8 floats behind every output row, a guard row above and below

            def framed():
                return torch.full((m + 2, ldo), NAN, device="cuda")

            def args(mx, out_ptr, ld):
                a = L.LinArgs()
                a.x, a.ldx, a.m, a.n, a.k = x.data_ptr(), k, m, n, k
                a.flags = L.LIN_W_FRAG
                a.out, a.ldo = out_ptr, ld
                a.pro, a.eps = pro, 1e-5
                if pro == 1:
                    a.norm_w = nw.data_ptr()
                if mod:
                    a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
                f = fx if mx else fb
                a.wdt = L.VV_MXFP6_FRAG if mx else L.VV_BF16
                a.w = f[1].data_ptr()
                if mx:
                    a.wscale = f[1].data_ptr() + n * k * 3 // 4
                if dual:
                    a.w2, a.act = f[2].data_ptr(), 2
                    if mx:
                        a.w2scale = f[2].data_ptr() + n * k * 3 // 4
                if epi:
                    a.gate, a.gate_ld, a.res, a.ldres = gate.data_ptr(), n, res.data_ptr(), n
                else:
                    a.bias = b.data_ptr()
                return a

            name = C.create_string_buffer(192)
            o1, o2, o16 = framed(), framed(), torch.zeros(m, n, device="cuda")
            L.check(lib.vv_linear_route(C.byref(args(True, o1[1].data_ptr(), ldo)), name, 192), "vv_linear_route")
            assert name.value.decode() == want_route, (name.value.decode(), want_route)
            s = torch.cuda.current_stream().cuda_stream
            L.check(lib.vv_linear(C.byref(args(True, o1[1].data_ptr(), ldo)), s), "vv_linear mxfp6")
            L.check(lib.vv_linear(C.byref(args(True, o2[1].data_ptr(), ldo)), s), "vv_linear mxfp6 again")      # the tickets must have been left ready
            L.check(lib.vv_linear(C.byref(args(False, o16.data_ptr(), n)), s), "vv_linear bf16")
            torch.cuda.synchronize()
            for o in (o1, o2):
                assert torch.isnan(o[0]).all() and torch.isnan(o[m + 1]).all() and torch.isnan(o[1: m + 1, n:]).all(), "a guard row or a gap was written"
            assert all(torch.equal(t.view(torch.uint8) if t.dtype != torch.uint8 else t, c.view(torch.uint8) if c.dtype != torch.uint8 else c)
                       for t, c in zip(inputs, kept)), "an input changed"
            o6 = o1[1: m + 1, :n].contiguous()
            assert torch.isfinite(o6).all()
            nd = int((o6.view(torch.int32) != o2[1: m + 1, :n].contiguous().view(torch.int32)).sum())
            assert nd == 0, f"{case} m={m}: two launches differ in {nd} outputs (ticketed fold: the order is fixed)"
            e = rel_rms(o6.double().cpu().numpy(), o16.double().cpu().numpy())
            print(f"{case} m={m}: mxfp6-frag vs bf16-frag rel RMS {e:.3e}")
            assert e < 1e-6, f"mxfp6-frag vs bf16-frag {case} m={m}: rel RMS {e:.3e}"
            xd = x.double()
            if pro == 1:
                xd = xd * torch.rsqrt((xd * xd).mean(-1, keepdim=True) + 1e-5) * nw.double()
                if mod:
                    xd = xd * (1 + sc.double()) + sh.double()
            y = xd @ e1.double().T
            if not epi:
                y = y + b.double()
            if dual:
                y = torch.nn.functional.silu(y) * (xd @ e2.double().T)
            if epi:
                y = y * gate.double() + res.double()
            err = rel_rms(o6.double().cpu().numpy(), y.cpu().numpy(), what=f"rows GEMV MXFP6 fragment-major {case} m={m} n={n} k={k} dual={dual} vs fp64 torch")
            print(f"{case} m={m}: vs fp64 rel RMS {err:.3e}")
            assert err < 2e-5, f"mxfp6 rows GEMV {case} m={m}: rel RMS {err:.3e}"
            if epi and k > 2048 and not pro:      # the atomic form: K slices, a linear epilogue, no prologue, res == out
                lib.vv_tune(b"gemv_rows_atomic", 1)
                out2 = res.clone()
                a = args(True, out2.data_ptr(), n)
                a.res = out2.data_ptr()
                L.check(lib.vv_linear_route(C.byref(a), name, 192), "vv_linear_route")
                assert name.value.decode() == route_of_case(case, atomic=True)[0] and name.value.decode().endswith("atomic=1"), name.value
                L.check(lib.vv_linear(C.byref(a), s), "vv_linear atomic")
                torch.cuda.synchronize()
                err = rel_rms(out2.double().cpu().numpy(), y.cpu().numpy())
                print(f"{case} m={m}: in place (atomic) vs fp64 rel RMS {err:.3e}")
                assert err < 2e-5, f"mxfp6 rows GEMV in place (atomic) {case} m={m}: rel RMS {err:.3e}"
    finally:
        lib.vv_tune(b"gemv_rows_scratch", 0)


# ---------------------------------------------------------------------------------------------------------------
# 2. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    """m <= 2, m > 8, a missing scale pointer (of w, of w2), a misaligned pointer (codes, scales), VV_LIN_X_BF16 / VV_LIN_OUT_BF16,
    VV_LIN_W_MXGEMM, the flag missing, n % 16, k % 128, K > 2048 without scratch: VV_E_UNSUPPORTED from vv_linear itself (and from
    vv_linear_route), the output untouched; the same call without the fault runs.  VV_MXFP6 keeps refusing the flag and 3 rows."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.weights import DeviceWeights, quantize_mxfp6
    n, k = 64, 1024
    c, s, _ = quantize_mxfp6(torch.randn(n, k))
    f = DeviceWeights.frag_major_mxfp6(c, s)
    f = torch.cat([f, f]).cuda()                                         # room behind every offset pointer below
    p, q = f.data_ptr(), f.data_ptr() + n * k * 3 // 4
    x = torch.randn(12, k, device="cuda")
    out = torch.full((12, n), NAN, device="cuda")
    name = C.create_string_buffer(192)

    def args(m=4, nn=n, kk=k, flags=L.LIN_W_FRAG, wdt=L.VV_MXFP6_FRAG, **kw):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo, a.flags = x.data_ptr(), k, m, nn, kk, wdt, out.data_ptr(), n, flags
        a.w, a.wscale = p, q
        for fld, v in kw.items():
            setattr(a, fld, v)
        return a

    dual = dict(w2=p, w2scale=q, act=L.ACT_SWIGLU)
    refused = {"m=1": args(1), "m=2": args(2), "m=9": args(9), "m=12": args(12), "no wscale": args(wscale=None), "no w2scale": args(**{**dual, "w2scale": None}),
               "w+8": args(w=p + 8), "wscale+2": args(wscale=q + 2), "w2+8": args(**{**dual, "w2": p + 8}), "w2scale+2": args(**{**dual, "w2scale": q + 2}),
               "x bf16": args(flags=L.LIN_W_FRAG | L.LIN_X_BF16), "out bf16": args(flags=L.LIN_W_FRAG | L.LIN_OUT_BF16), "no flag": args(flags=0),
               "mxgemm": args(flags=L.LIN_W_FRAG | L.LIN_W_MXGEMM), "n%16": args(nn=56), "k%128": args(kk=k - 64),
               "mxfp6 + flag, 4 rows": args(wdt=L.VV_MXFP6), "mxfp6, 3 rows": args(3, flags=0, wdt=L.VV_MXFP6)}
    for what, a in refused.items():
        rc_route = lib.vv_linear_route(C.byref(a), name, 192)
        rc_run = lib.vv_linear(C.byref(a), None)
        assert rc_route == rc_run == VV_E_UNSUPPORTED and name.value == b"", (what, rc_route, rc_run, lib.vv_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its output"
    for a in (args(), args(3), args(8, **dual)):
        assert lib.vv_linear_route(C.byref(a), name, 192) == 0 and name.value.decode().startswith("gemv_rows_mx6<"), lib.vv_last_error()
        assert lib.vv_linear(C.byref(a), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out[:8]).all() and torch.isnan(out[8:]).all()
    # beyond K = 2048 the K slices need scratch (or the in-place atomic form): refused without, the output untouched
    k2 = 4096
    c, s, _ = quantize_mxfp6(torch.randn(n, k2))
    f2 = DeviceWeights.frag_major_mxfp6(c, s).cuda()
    x2 = torch.randn(4, k2, device="cuda")
    out.fill_(NAN)
    a = args(kk=k2, x=x2.data_ptr(), ldx=k2, w=f2.data_ptr(), wscale=f2.data_ptr() + n * k2 * 3 // 4)
    assert lib.vv_linear_route(C.byref(a), name, 192) == lib.vv_linear(C.byref(a), None) == VV_E_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---------------------------------------------------------------------------------------------------------------
# 3. the engine at `mid`
# ---------------------------------------------------------------------------------------------------------------
class _Tok:
    def __init__(self, vocab, pad=None):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = vocab - 4, vocab - 3, vocab - 2, vocab - 1
        self.bos_token_id = None
        self.pad_id = vocab - 5 if pad is None else pad


MID_SEED = 4321


def _mid_model(**kw):
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg = VVConfig.preset("mid")
    m = VibeVoiceForConditionalGenerationInference.from_synthetic(cfg, MID_SEED, device="cuda:0", torch_dtype=torch.bfloat16, numpy_weights=True,
                                                                  weight_quant="mxfp6", **kw)
    m.set_ddpm_inference_steps(N_STEPS)
    return cfg, m


def _idle_streams_back(m=None):
    """drop the lanes of `m` (if given) and collect dead engines now: their streams go back to the recycle pool (engine.py, _IDLE_STREAMS)"""
    if m is not None:
        m.release_lanes()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def mid():
    """the opt-in model at `mid`, shared by the engine tests.  An engine takes its HIP stream from the package's recycle pool and draws a new one
    from torch only when that pool is empty - and torch hands out 32 streams round-robin, so every extra draw shifts which stream the lanes of
    all later tests get, until two lanes that capture side by side share one.  This module must therefore draw none: engines that earlier
    modules left for the garbage collector hand their streams back before the model is built (_idle_streams_back), and the model is torn down
    here, its own streams back in the pool, when the module ends."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    _idle_streams_back()
    box = list(_mid_model(mxfp6_row_batch=True))      # [cfg, model]: a list, so that the fixture's cached value does not keep the model alive below
    yield box
    box.pop().release_lanes()
    gc.collect()
    torch.cuda.empty_cache()


def _companion_shapes(cfg):
    """(n, k) of every matrix that has an MXFP6 companion on the LLM and head path, by f_* name"""
    qkvd, hd = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, cfg.heads * cfg.head_dim
    llm = {"qkv": (qkvd, cfg.hidden), "o": (cfg.hidden, hd), "gate": (cfg.inter, cfg.hidden), "up": (cfg.inter, cfg.hidden), "down": (cfg.hidden, cfg.inter)}
    head = {"gate": (cfg.head_ffn, cfg.head_hidden), "up": (cfg.head_ffn, cfg.head_hidden), "down": (cfg.head_hidden, cfg.head_ffn)}
    return llm, head


def _mx6_frag_ptrs(w):
    """every f_* pointer of the LLM and head layers: a uint8 VV_MXFP6_FRAG copy (planes A and B + scale bytes) where the shape fits, NULL
    elsewhere - and for the head's gate / up pair beyond K = 2048, which no MX rows route takes with its adaLN prologue (7B widths)"""
    by_ptr = {t.data_ptr(): t for t in w._frag_state["tensors"]}
    llm, head = _companion_shapes(w.cfg)
    ptrs = []
    for lay, shapes in [(w.llm.layer[l], llm) for l in range(w.cfg.layers)] + [(w.head.layer[l], head) for l in range(w.cfg.head_layers)]:
        for nm, (n, k) in shapes.items():
            p = getattr(lay, "f_" + nm)
            if n % 16 or k % 128 or (shapes is head and nm in ("gate", "up") and k > 2048):
                assert not p
                continue
            assert p and by_ptr[p].dtype == torch.uint8 and by_ptr[p].numel() == n * k * 25 // 32, f"f_{nm}"
            ptrs.append(p)
    assert all(t.dtype == torch.uint8 for t in w._frag_state["tensors"]), "a bf16 fragment copy next to the MXFP6 ones"
    return ptrs


def test_decode_step_8_rows_mxfp6_vs_batch2(mid):
    """One row-batched MXFP6 decode step (8 rows on the fragment-major codes) against the MXFP6 batch-2 step (1..2-row streaming GEMV) of every
    dialogue on its own engine state: hidden rows, constrained logits, tokens, positions.  Bars of test_decode_step_8_rows_mxfp4_vs_batch2."""
    _decode_step_vs_batch2(*mid, "mid")


def _decode_step_vs_batch2(cfg, m, tag):
    from vibevoice_rocm_amd.rowbatch import RowBatch
    tok = _Tok(cfg.vocab)
    ST, SD = tok.speech_start_id, tok.speech_diffusion_id
    valid = [ST, tok.speech_end_id, SD, tok.eos_token_id]
    B = 4
    lanes = [m._lane(b) for b in range(B)]
    rb = RowBatch(lanes)
    _mx6_frag_ptrs(m.engine.w)
    g = torch.Generator().manual_seed(17)
    lens = [50, 37, 44, 29]
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([ST])]) for n in lens]
    rb.begin(128, valid, 2.0)
    ref_h, ref_tok, ref_logits, ref_lens = [], [], [], []
    eng = m.engine
    for b in range(B):
        eng.begin_sequence(128, valid)
        x0 = eng.embed_ids(prompts[b])
        eng.prefill(x0, row=0, pos0=0)
        t0 = eng.first_token(ST, SD, SD)
        eng.prefill(eng.embed_ids(torch.tensor([ST])), row=1, pos0=0)
        with torch.cuda.stream(eng.stream):
            xin = torch.randn(cfg.hidden, generator=g).cuda() * 0.5
            eng.x2[0].copy_(xin); eng.x2[1].copy_(xin)
        t1 = eng.step_decode(ST, SD, None)
        eng.stream.synchronize()
        ref_h.append(eng.hidden2.clone()); ref_tok.append(t1); ref_logits.append(eng.logits[:4].clone()); ref_lens.append(eng.lens.clone())
        rb.prefill(b, x0)
        assert rb.first_token(b, SD) == t0 == SD
        rb.prefill(b, eng.embed_ids(torch.tensor([ST])), neg=True)
        with torch.cuda.stream(rb.stream):
            rb.x[2 * b].copy_(xin); rb.x[2 * b + 1].copy_(xin)
    rb.decode_begin(ST, SD, {b: None for b in range(B)})
    toks = rb.decode_end()
    rb.synchronize()
    for b in range(B):
        eh = rel_rms(rb.hidden[2 * b: 2 * b + 2].cpu().numpy(), ref_h[b].cpu().numpy(),
                     what=f"row-batched mxfp6 decode step {tag}, dialogue {b} of 4: hidden rows vs the mxfp6 batch-2 step")
        el = rel_rms(rb.logits[b, :4].cpu().numpy(), ref_logits[b].cpu().numpy())
        print(f"{tag} dialogue {b}: hidden {eh:.3e} logits {el:.3e}")
        assert eh < 5e-3 and el < 5e-3, f"dialogue {b}: hidden {eh:.3e} logits {el:.3e}"
        assert toks[b] == ref_tok[b]
        assert rb.lens[2 * b: 2 * b + 2].tolist() == ref_lens[b].tolist()
    rb.close()


@pytest.mark.parametrize("solver", ["ode", "sde"])
def test_head_sample_batch_mxfp6_vs_single(mid, solver):
    """The batched head sampler (4 utterances, 8 rows per pass over the MXFP6 fragment-major codes) against the MXFP6 single-utterance sampler,
    under the ODE and the SDE solver.  Bar of test_head_sample_batch_mxfp4_vs_single."""
    cfg, m = mid
    eng = m.engine
    lb = eng.lib
    eng.w.ensure_frag()
    _mx6_frag_ptrs(eng.w)
    ode = m.model.noise_scheduler
    if solver == "sde":
        m.model.noise_scheduler = ode.from_config(ode.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")
        m.set_ddpm_inference_steps(N_STEPS)
        assert eng.sde
    try:
        B = 4
        g = torch.Generator().manual_seed(11 if solver == "ode" else 12)
        cond = torch.randn(2 * B, cfg.hidden, generator=g).cuda()
        noise = torch.randn(B, cfg.latent, generator=g).cuda()
        sde_noise = torch.randn(B, N_STEPS, cfg.latent, generator=g).cuda() if solver == "sde" else None
        with torch.cuda.stream(eng.stream):
            lat = torch.zeros(B, cfg.latent, device="cuda")
            if solver == "sde":
                ws = torch.empty(lb.vv_head_ws_bytes_batch_sde(C.byref(eng.w.head), N_STEPS, B), dtype=torch.uint8, device="cuda")
                eng._ck(lb.vv_head_sample_batch_sde(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(),
                                                    eng._coefs, N_STEPS, 2.0, lat.data_ptr(), cfg.latent, B, ws.data_ptr(), sde_noise.data_ptr(),
                                                    N_STEPS * cfg.latent, eng.sp), "vv_head_sample_batch_sde")
            else:
                ws = torch.empty(lb.vv_head_ws_bytes_batch(C.byref(eng.w.head), N_STEPS, B), dtype=torch.uint8, device="cuda")
                eng._ck(lb.vv_head_sample_batch(C.byref(eng.w.head), cond.data_ptr(), cfg.hidden, noise.data_ptr(), cfg.latent, eng.temb.data_ptr(),
                                                eng._coefs, N_STEPS, 2.0, lat.data_ptr(), cfg.latent, B, ws.data_ptr(), eng.sp), "vv_head_sample_batch")
            one = torch.zeros(B, cfg.latent, device="cuda")
            for b in range(B):
                eng._ck(lb.vv_head_sample(C.byref(eng.w.head), cond[2 * b:].data_ptr(), cfg.hidden, noise[b].data_ptr(), eng.temb.data_ptr(), eng._coefs,
                                          N_STEPS, 2.0, one[b].data_ptr(), eng._head_ws.data_ptr(),
                                          None if sde_noise is None else sde_noise[b].data_ptr(), eng.sp), "vv_head_sample")
        eng.stream.synchronize()
        assert torch.isfinite(lat).all()
        for b in range(B):
            err = rel_rms(lat[b].cpu().numpy(), one[b].cpu().numpy(),
                          what=f"row-batched mxfp6 head sampling ({solver}) mid, utterance {b} of 4, vs the mxfp6 single-utterance sampler")
            print(f"{solver} utterance {b}: {err:.3e}")
            assert err < 2e-3, f"{solver} utterance {b}: rel RMS {err:.3e}"
    finally:
        m.model.noise_scheduler = ode
        m.set_ddpm_inference_steps(N_STEPS)


def _padded(tok, lens, g):
    S = tok.speech_start_id
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([S])]) for n in lens]
    Lp = max(lens)
    ids = torch.stack([torch.cat([torch.full((Lp - n,), tok.pad_id), p]) for n, p in zip(lens, prompts)])
    mask = torch.stack([torch.cat([torch.zeros(Lp - n, dtype=torch.long), torch.ones(n, dtype=torch.long)]) for n in lens])
    return ids, mask, prompts


@pytest.fixture(scope="module")
def oracle_weights():
    """the state dict the oracle computes with: MXFP6 effective weights for the companion-set matrices, bf16 roundings for the other matrices"""
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    from vibevoice_rocm_amd.weights import fp8_matrix_names, mxfp6_effective_state_dict
    cfg = VVConfig.preset("mid")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, MID_SEED).items()}
    eff = mxfp6_effective_state_dict(cfg, sd)
    names = set(fp8_matrix_names(cfg))
    return {k: (eff[k] if k in names else (v.to(torch.bfloat16).float() if v.dim() >= 2 else v)) for k, v in sd.items()}


@pytest.mark.parametrize("B", [3, 4])
def test_generate_mxfp6_row_batch_vs_lanes_and_oracle(mid, oracle_weights, B):
    """generate() on 3 and on 4 dialogues with different prompt lengths and token schedules (an early end, a turn switch).  The opt-in takes the
    row batch; row_batch=False keeps the lanes on the same weights: same sequences, waveforms under 1e-2 (the bar of
    test_generate_mxfp4_row_batch_vs_lanes).  Each dialogue of the row batch against the CPU oracle on mxfp6_effective_state_dict under 2e-2
    (the bar of test_generate_mxfp4_row_batch_mid_vs_oracle)."""
    from oracle import vv_oracle as O
    cfg, m = mid
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(64 + B)
    ids, mask, prompts = _padded(tok, [40, 31, 36, 27][:B], g)
    forced = [[D] * 5 + [E, EOS], [D] * 3 + [E, S, D, D, E, EOS], [D] * 2 + [E, EOS], [D] * 4 + [E, EOS]][:B]
    noise = torch.randn(B, 8, cfg.latent, generator=g)
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    steps = 10                                   # the oracle runs on the CPU: 10 solver steps keep each case to a few seconds
    m.release_lanes()
    m.set_ddpm_inference_steps(steps)
    try:
        lanes = m.generate(row_batch=False, **kw)
        assert not m._rowbatch, "row_batch=False took the row-batched path"
        rows = m.generate(**kw)
    finally:
        m.set_ddpm_inference_steps(N_STEPS)
    assert (B, 0) in m._rowbatch, f"mxfp6_row_batch=True on {B} dialogues did not take the row-batched path"
    _mx6_frag_ptrs(m.engine.w)
    assert rows.sequences.tolist() == lanes.sequences.tolist()
    special = dict(speech_start=S, speech_end=E, speech_diffusion=D, eos=EOS)
    for b in range(B):
        a, r = rows.speech_outputs[b], lanes.speech_outputs[b]
        assert a.shape == r.shape
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what=f"generate() mxfp6 on {B} dialogues mid, row-batched vs lanes, waveform of dialogue {b}")
        n_p = prompts[b].numel()
        ref = O.generate(oracle_weights, cfg.as_dict(), prompts[b].tolist(), torch.zeros(n_p, dtype=torch.bool), None, special, noise[b], cfg_scale=2.0,
                         n_steps=steps, forced_tokens=forced[b], bf16_t=True)
        eo = rel_rms(a.float().cpu().numpy().reshape(-1), torch.cat(ref.audio).numpy().reshape(-1),
                     what=f"generate() mxfp6 on {B} dialogues mid, ROW-BATCHED vs oracle on the effective weights, dialogue {b}")
        print(f"B={B} dialogue {b}: row-batched vs lanes {err:.3e}, vs oracle {eo:.3e}")
        assert err < 1e-2, f"dialogue {b}: waveform rel RMS {err:.3e} vs lanes"
        assert eo < 2e-2, f"dialogue {b}: waveform rel RMS {eo:.3e} vs oracle"


def test_row_batch_streams_mxfp6_frag_for_every_companion_matrix(mid):
    """Under vv_prof_begin / vv_prof_end an eager row-batched generate() on 3 dialogues (6 rows) records, for every matrix that has a companion
    and K % 128 == 0, launches with wdt == VV_MXFP6_FRAG at 6 rows - once per layer per decode step, once per head layer per solver step per
    sampler call at least - and no bf16 launch of that matrix in that row range.  At `mid` the o projection shares its shape [512, 512] with the
    head's cond_proj (no companion: bf16, once per sampler call): its bf16 count must be exactly the number of sampler calls."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    lb = L.load()
    _idle_streams_back(mid[1])           # the shared model's lanes hand their streams to the second model built here
    cfg, m = _mid_model(mxfp6_row_batch=True, use_graphs=False)
    steps = 10
    m.set_ddpm_inference_steps(steps)
    tok = _Tok(cfg.vocab)
    D, E, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id
    g = torch.Generator().manual_seed(16)
    ids, mask, _ = _padded(tok, [24, 20, 22], g)
    forced = [[D, D, D, E, EOS]] * 3
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=torch.randn(3, 4, cfg.latent, generator=g))
    m.generate(**kw)
    assert (3, 0) in m._rowbatch
    L.check(lb.vv_prof_begin(200000), "vv_prof_begin")
    try:
        m.generate(**kw)
    finally:
        ents = (L.ProfEntry * 1024)()
        cnt = C.c_int(0)
        L.check(lb.vv_prof_end(ents, 1024, C.byref(cnt)), "vv_prof_end")
    rec = [ents[i] for i in range(cnt.value)]
    mx, bf = {}, {}
    for e in rec:
        if e.wdt == L.VV_MXFP6_FRAG:
            assert e.m == 6
            mx[(e.n, e.k, e.dual)] = mx.get((e.n, e.k, e.dual), 0) + e.count
        elif e.wdt == L.VV_BF16 and 3 <= e.m <= 8:
            bf[(e.n, e.k, e.dual)] = bf.get((e.n, e.k, e.dual), 0) + e.count
    llm, head = _companion_shapes(cfg)
    assert all(k % 128 == 0 and n % 16 == 0 for n, k in list(llm.values()) + list(head.values()))
    decodes, frames = len(forced[0]) - 1, 3
    want = {}
    for key, count in (((*llm["qkv"], 0), cfg.layers * decodes), ((*llm["o"], 0), cfg.layers * decodes), ((*llm["gate"], 1), cfg.layers * decodes),
                       ((*llm["down"], 0), cfg.layers * decodes), ((*head["gate"], 1), cfg.head_layers * steps * frames),
                       ((*head["down"], 0), cfg.head_layers * steps * frames)):
        want[key] = want.get(key, 0) + count
    for key, least in want.items():
        assert mx.get(key, 0) >= least, f"{key}: {mx.get(key, 0)} VV_MXFP6_FRAG launches at 6 rows, expected at least {least}"
    assert llm["gate"] == head["gate"] and llm["o"] == (cfg.head_hidden, cfg.hidden), "the shape bookkeeping below is for `mid`"
    steps_a = mx[(*llm["qkv"], 0)] // cfg.layers                                          # row-batched decode steps
    calls_h = (mx[(*llm["gate"], 1)] - cfg.layers * steps_a) // (cfg.head_layers * steps)  # batched sampler calls
    assert steps_a >= decodes and calls_h >= frames
    for key in want:
        if key == (*llm["o"], 0):
            assert bf.get(key, 0) == calls_h, f"{key}: {bf.get(key, 0)} bf16 launches at 3..8 rows, the head's cond_proj accounts for {calls_h}"
        else:
            assert bf.get(key, 0) == 0, f"{key}: {bf[key]} bf16 launches at 3..8 rows next to the MXFP6 fragment copies"
    m.release_lanes()
    del m
    gc.collect()
    torch.cuda.empty_cache()


def test_fragment_copies_are_built_once(mid):
    """A 3-dialogue call, then a 6-dialogue call (two row batches, the second led by a forked lane): the MXFP6 fragment copies are built once
    for the weights and every fork; the VRAM record is 0.78125 bytes per copied weight, as nbytes() counts it."""
    cfg, m = mid
    tok = _Tok(cfg.vocab)
    D, E, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id
    g = torch.Generator().manual_seed(3)
    m.set_ddpm_inference_steps(10)

    def call(B):
        ids, mask, _ = _padded(tok, [20 + b for b in range(B)], g)
        m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=[[D, D, E, EOS]] * B,
                   noise=torch.randn(B, 4, cfg.latent, generator=g))

    try:
        m.release_lanes()
        call(3)
        assert (3, 0) in m._rowbatch
        w = m.engine.w
        ptrs = _mx6_frag_ptrs(w)
        n_frag = len(w._frag_state["tensors"])
        call(6)
        assert len(m._rowbatch) >= 2
        torch.cuda.synchronize()
        assert _mx6_frag_ptrs(w) == ptrs and len(w._frag_state["tensors"]) == n_frag
        mem = torch.cuda.memory_allocated()
        for e in m._lanes:
            e.w.ensure_frag()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == mem, "a forked lane built its own fragment copies"
        llm, head = _companion_shapes(cfg)
        weights = cfg.layers * sum(n * k for n, k in llm.values()) + cfg.head_layers * sum(n * k for n, k in head.values())
        st = w._frag_state
        assert st["mxfp6_weights"] == weights and st["mxfp6_bytes"] == weights * 25 // 32 == sum(t.numel() for t in st["tensors"])
    finally:
        m.set_ddpm_inference_steps(N_STEPS)


# ---------------------------------------------------------------------------------------------------------------
# 4. a session
# ---------------------------------------------------------------------------------------------------------------
def test_session_mxfp6_vs_generate_alone(mid):
    """open_session on the opt-in model, two slots: two requests with different cfg_scale, lengths and schedules, each against generate() on it
    alone (the single-dialogue MXFP6 engine) at the bar of test_session_mxfp4_vs_generate_alone (1e-2)."""
    cfg, m = mid
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(61)
    lens, scales = [44, 30], [1.3, 3.0]
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([S])]) for n in lens]
    forced = [[D] * 6 + [E, EOS], [D] * 3 + [E, S] + [D] * 2 + [E, EOS]]
    noise = torch.randn(2, 8, cfg.latent, generator=g)
    m.release_lanes()
    with m.open_session(tokenizer=tok, slots=2, max_context=256, device_noise=False) as sess:
        hs = [sess.submit(input_ids=prompts[i][None], cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i]) for i in range(2)]
        sess.run()
    assert m._session is None and all(h.done for h in hs) and [h.slot for h in hs] == [0, 1]
    _mx6_frag_ptrs(m.engine.w)
    for i in range(2):
        want = m.generate(input_ids=prompts[i][None], tokenizer=tok, cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i])
        got = hs[i].result()
        assert got.sequences.tolist() == want.sequences.tolist() == [prompts[i].tolist() + forced[i]]
        err = rel_rms(got.speech_outputs[0].float().cpu().numpy(), want.speech_outputs[0].float().cpu().numpy(),
                      what=f"session of 2 slots, mid mxfp6, dialogue {i} (cfg {scales[i]}, slot {hs[i].slot}) vs generate() alone")
        print(f"session dialogue {i} slot {hs[i].slot}: waveform rel RMS {err:.3e}")
        assert err < 1e-2, f"dialogue {i}: waveform rel RMS {err:.3e}"


# ---------------------------------------------------------------------------------------------------------------
# 5. the 7B widths
# ---------------------------------------------------------------------------------------------------------------
def test_decode_step_8_rows_mxfp6_7b_widths_vs_batch2(mid):
    """7B widths (H 3584, I 18944; 2 LLM layers): the 8-row step - qkv / o on K splits, the SwiGLU pair on a 2-slice split, the down projection on
    13 slices folded through tickets or added in place - against the batch-2 MXFP6 step, GPU against GPU."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    _idle_streams_back(mid[1])
    cfg = dataclasses.replace(VVConfig.preset("7b"), layers=2)
    sd = synth_state_dict_torch(cfg, 778, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp6", mxfp6_row_batch=True)
    del sd
    try:
        _decode_step_vs_batch2(cfg, m, "7B widths")
    finally:
        m.release_lanes()
        del m
        gc.collect()
        torch.cuda.empty_cache()
