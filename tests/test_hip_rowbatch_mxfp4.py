"""GPU parity of MXFP4 on the row-batched decode path (weight_quant="mxfp4", mxfp4_row_batch=True; csrc/vv_gemv_rows.hip).

1. the kernel: decode read back exactly (every code in every nibble position, scale bytes 2 / 127 / 252), then vv_linear on VV_MXFP4_FRAG codes
   against vv_linear on the bf16 fragment-major copy of the effective matrix - bit for bit wherever both forms cut K alike (ticketed split,
   deterministic), to fp32 reassociation (rel RMS < 1e-6) where they do not (SPLIT_DIFFERS, derived from both decisions) -, against fp64 torch
   (< 2e-5) and in place with the atomic split (< 2e-5): the bars of test_rows_gemv_fp8_frag_vs_bf16_frag.  m in {3, 5, 8}; the smallest shapes
   that reach every compiled instantiation in every form (CASES); every case twice, so tickets are proven to be left ready.
2. refusals: VV_E_UNSUPPORTED from vv_linear_route and vv_linear alike, nothing written.
3. the engine at `mid`: the 8-row decode step against the batch-2 MXFP4 step, the batched head sampler against the single one, generate() row
   batch against lanes and against the oracle on the effective weights, the profiler record, the fragment copies built once.
4. a session on that model.  5. the 7B widths (2 layers), GPU against GPU.
Measured errors go into the parity record (conftest.rel_rms `what=`)."""
import ctypes as C
import dataclasses
import gc

import pytest
import torch

from conftest import rel_rms
from test_host_rowbatch_mxfp4 import ALL_ROWS_MX, rows_bf16_cut, rows_mx_decide

pytestmark = pytest.mark.gpu

VV_E_UNSUPPORTED = -3
N_STEPS = 20
MX_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


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


# ---------------------------------------------------------------------------------------------------------------
# 1. the kernel
# ---------------------------------------------------------------------------------------------------------------
# (n, k, dual, rms prologue, adaLN, gate + residual epilogue (else bias), hooks): the smallest shapes that reach every instantiation and form
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
    "split_ks2_k4608": (48, 4608, 0, 0, 0, 1, {"gemv_rows_blocks": 15}),  # 5 slices of 2 loads per wave, the last ragged (the 1.5B head's down projection's cut)
    "split_ks3_k4608": (48, 4608, 0, 1, 0, 0, {"gemv_rows_blocks": 9}),   # 3 slices of 3 loads per wave
    "split_ks4_k18944": (32, 18944, 0, 0, 0, 1, {}),                      # the 7B down projection's K: 10 slices of 4 loads, the last ragged
    "dual_split_k2176": (32, 2176, 1, 1, 0, 0, {}),                       # SwiGLU K split: 3 slices, the last holds one load
    "dual_split_ks2_k3584": (32, 3584, 1, 1, 0, 0, {"gemv_rows_blocks": 1}),   # the 7B gate / up cut: 2 slices of 2 loads per wave
}
# the cases whose bf16 form cuts K another way (other waves, other slices): same products, another summation order
SPLIT_DIFFERS = {"one_load_k128", "one_load_k384_ragged", "dual_k512", "dual_adaln_k1536", "split_k2176_ragged", "split_k4608_rms",
                 "split_ks3_k4608", "split_ks4_k18944", "dual_split_k2176", "dual_split_ks2_k3584"}


def _route(case):
    n, k, dual, pro, mod, epi, hooks = CASES[case]
    return rows_mx_decide(n, k, dual, mod=bool(mod), blocks=hooks.get("gemv_rows_blocks", 448), pers=hooks.get("gemv_rows_pers", 192))


def test_cases_reach_every_compiled_instantiation_and_form():
    """The cases' routes (restated decision) are the 10 kernels of the unit, whole-row, persistent and K-split forms with ragged ends included;
    SPLIT_DIFFERS is exactly the set of cases whose K cut differs from the bf16 form's."""
    routes = {c: _route(c) for c in CASES}
    assert all(r is not None for r in routes.values())
    assert {r[0].split(" ")[0] for r in routes.values()} == set(ALL_ROWS_MX)
    differs = {c for c, (n, k, dual, pro, mod, epi, hooks) in CASES.items()
               if routes[c][1] != rows_bf16_cut(n, k, dual, blocks=hooks.get("gemv_rows_blocks", 448))}
    assert differs == SPLIT_DIFFERS, sorted(differs ^ SPLIT_DIFFERS)
    # bit for bit: whole rows of 8 x 8 steps, the persistent walk at 8 x 4 steps, and a ticketed K split of 5 slices x 4 waves x 8 steps
    assert set(CASES) - SPLIT_DIFFERS == {"whole_row_k2048", "dual_pers_k2048", "dual_pers_k1024", "split_ks2_k4608"}
    ragged = [c for c in CASES if routes[c][1][0] * routes[c][1][1] * routes[c][1][2] * 32 > CASES[c][1]]
    assert {"one_load_k384_ragged", "split_k2176_ragged", "split_ks4_k18944", "dual_split_k2176"} <= set(ragged)


def _planted(n, k, seed, x_free_block):
    """MXFP4 codes [n, k] / scale bytes [n, k / 32] of a random matrix with all 16 codes (-0 = code 8 included) planted in every row and scale
    bytes 2, 127 and 252 planted in blocks 1, 2 and `x_free_block` of rows 1, 17, ...; returns (codes, scales, effective matrix bf16 - exact)"""
    from vibevoice_rocm_amd.weights import quantize_mxfp4
    g = torch.Generator(device="cuda").manual_seed(seed)
    codes, scales, _ = quantize_mxfp4((torch.randn(n, k, device="cuda", generator=g) / k ** 0.5).bfloat16())
    rows = torch.arange(n, device="cuda")
    for c in range(16):
        codes[rows, (rows * 5 + c * 7 + 3) % 32] = c                 # 16 distinct columns of block 0 (7 is a unit mod 32), shifted per row
    nb = k // 32
    scales[1::16, 1 % nb] = 2
    scales[1::16, 2 % nb] = 127
    scales[1::16, x_free_block] = 252
    val = torch.tensor(MX_VALUES + tuple(-v for v in MX_VALUES), device="cuda", dtype=torch.float64)
    eff = val[codes.long()] * torch.exp2(scales.double() - 127).repeat_interleave(32, dim=1)
    eff16 = eff.bfloat16()
    assert torch.equal(eff16.double(), eff), "value(code) * 2^(e - 127) must be exact in bf16"
    return codes.contiguous(), scales.contiguous(), eff16


def test_decode_is_exact(lib):
    """Every weight of a [32, 256] matrix read back through the kernel with one-hot activations (8 columns per launch): all 16 codes in every
    nibble position, scale bytes 2, 64, 127, 200 and 252 - each output is value(code) * 2^(e - 127) bit for bit (a zero weight reads +0).  Pins
    nibble order, dword / k-step order, lane assignment, and scale byte placement."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.weights import DeviceWeights
    n, k = 32, 256
    r, c = torch.arange(n)[:, None], torch.arange(k)[None, :]
    codes = ((r * 3 + c + c // 8) % 16).to(torch.uint8).cuda()
    scales = torch.tensor([2, 64, 127, 200, 252, 120, 134, 127], dtype=torch.uint8)[(torch.arange(n)[:, None] + torch.arange(k // 32)[None, :] * 3) % 8].cuda()
    f = DeviceWeights.frag_major_mxfp4(codes, scales)
    val = torch.tensor(MX_VALUES + tuple(-v for v in MX_VALUES), dtype=torch.float64, device="cuda")
    want = (val[codes.long()] * torch.exp2(scales.double() - 127).repeat_interleave(32, dim=1)).float()      # [n, k]
    want = torch.where(want == 0, torch.zeros_like(want), want)
    got = torch.empty(k, n, device="cuda")
    x = torch.zeros(k // 8, 8, k, device="cuda")
    for j in range(k // 8):
        x[j, torch.arange(8), 8 * j + torch.arange(8)] = 1.0
    for j in range(k // 8):
        a = L.LinArgs()
        a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.flags = x[j].data_ptr(), k, 8, n, k, L.VV_MXFP4_FRAG, L.LIN_W_FRAG
        a.w, a.wscale = f.data_ptr(), f.data_ptr() + n * k // 2
        a.out, a.ldo = got[8 * j:].data_ptr(), n
        L.check(lib.vv_linear(C.byref(a), torch.cuda.current_stream().cuda_stream), "vv_linear")
    torch.cuda.synchronize()
    bad = (got.t().contiguous().view(torch.int32) != want.view(torch.int32))
    assert not bad.any(), f"{int(bad.sum())} weights decode wrong, first at {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("m_rows", [3, 5, 8])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_gemv_mxfp4_frag_vs_bf16_frag(lib, case, m_rows):
    """vv_linear on VV_MXFP4_FRAG codes + scale bytes against vv_linear on the bf16 fragment-major copy of the effective matrix (ticketed split,
    every launch twice): IDENTICAL outputs where both forms cut K alike, rel RMS < 1e-6 where they do not (SPLIT_DIFFERS; measured <= 3.7e-7);
    then against fp64 torch (< 2e-5; measured <= 7.7e-6) and, for the K-split cases with a linear in-place epilogue, the atomic form (< 2e-5;
    measured <= 4.3e-6).  The route is the restated decision's.  Scale byte 252 sits in the last block of rows 1, 17, ...: its activations are
    bf16-exact multiples of 2^-125 (no prologue) or zero (a prologue would rescale them), so every product stays finite."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.weights import DeviceWeights
    n, k, dual, pro, mod, epi, hooks = CASES[case]
    m = m_rows
    want_route = _route(case)[0]
    L.check(lib.vv_tune(b"gemv_rows_scratch", 1), "scratch")
    try:
        with _tuned(lib, {**hooks, "gemv_rows_atomic": 0}):
            torch.manual_seed(m * 1000 + n + k)
            # the block of the scale byte 252 (weights up to 6 x 2^125): its activations are zero under a prologue (which rescales them) and
            # bf16-exact multiples of 2^-125 without one, so that its products are O(1) and exact in both forms
            xb = (k // 32) - 1
            x = torch.randn(m, k, device="cuda") * 1.5
            x[:, 32 * xb:] = 0.0 if pro else (1 + torch.randint(0, 128, (m, 32), device="cuda") / 128.0) * torch.where(torch.rand(m, 32, device="cuda") < 0.5, -1.0, 1.0) * 2.0 ** -125
            q1, s1, e1 = _planted(n, k, n + k, xb)
            q2, s2, e2 = _planted(n, k, n + k + 1, xb) if dual else (None, None, None)
            nw = torch.rand(k, device="cuda") + 0.5
            sh, sc = torch.randn(m, k, device="cuda") * 0.2, torch.randn(m, k, device="cuda") * 0.2
            sh[:, 32 * xb:] = 0.0
            gate, res, b = torch.randn(m, n, device="cuda"), torch.randn(m, n, device="cuda"), torch.randn(n, device="cuda")
            fx = {1: DeviceWeights.frag_major_mxfp4(q1, s1), 2: DeviceWeights.frag_major_mxfp4(q2, s2) if dual else None}
            fb = {1: DeviceWeights.frag_major(e1), 2: DeviceWeights.frag_major(e2) if dual else None}
            assert fx[1] is not None and fb[1] is not None and fx[1].data_ptr() % 16 == 0

            def args(mx, out):
                a = L.LinArgs()
                a.x, a.ldx, a.m, a.n, a.k = x.data_ptr(), k, m, n, k
                a.flags = L.LIN_W_FRAG
                a.out, a.ldo = out.data_ptr(), n
                a.pro, a.eps = pro, 1e-5
                if pro == 1:
                    a.norm_w = nw.data_ptr()
                if mod:
                    a.mod_shift, a.mod_scale, a.ld_mod = sh.data_ptr(), sc.data_ptr(), k
                f = fx if mx else fb
                a.wdt = L.VV_MXFP4_FRAG if mx else L.VV_BF16
                a.w = f[1].data_ptr()
                if mx:
                    a.wscale = f[1].data_ptr() + n * k // 2
                if dual:
                    a.w2, a.act = f[2].data_ptr(), 2
                    if mx:
                        a.w2scale = f[2].data_ptr() + n * k // 2
                if epi:
                    a.gate, a.gate_ld, a.res, a.ldres = gate.data_ptr(), n, res.data_ptr(), n
                else:
                    a.bias = b.data_ptr()
                return a

            name = C.create_string_buffer(192)
            L.check(lib.vv_linear_route(C.byref(args(True, res)), name, 192), "vv_linear_route")
            assert name.value.decode() == want_route, (name.value.decode(), want_route)
            s = torch.cuda.current_stream().cuda_stream
            o4, o16 = torch.zeros(m, n, device="cuda"), torch.zeros(m, n, device="cuda")
            for _ in range(2):          # twice: the split-K tickets must be left ready for the next launch
                L.check(lib.vv_linear(C.byref(args(True, o4)), s), "vv_linear mxfp4")
                L.check(lib.vv_linear(C.byref(args(False, o16)), s), "vv_linear bf16")
            torch.cuda.synchronize()
            assert torch.isfinite(o4).all()
            if case in SPLIT_DIFFERS:
                e = rel_rms(o4.double().cpu().numpy(), o16.double().cpu().numpy())
                print(f"{case} m={m}: mxfp4-frag vs bf16-frag (other K cut) rel RMS {e:.3e}")
                assert e < 1e-6, f"mxfp4-frag vs bf16-frag {case} m={m} (other K cut): rel RMS {e:.3e}"
            else:
                nd = int((o4 != o16).sum())
                assert nd == 0, f"mxfp4-frag vs bf16-frag {case} m={m}: {nd} outputs differ (max {(o4 - o16).abs().max().item():.3e})"
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
            err = rel_rms(o4.double().cpu().numpy(), y.cpu().numpy(), what=f"rows GEMV MXFP4 fragment-major {case} m={m} n={n} k={k} dual={dual} vs fp64 torch")
            print(f"{case} m={m}: vs fp64 rel RMS {err:.3e}")
            assert err < 2e-5, f"mxfp4 rows GEMV {case} m={m}: rel RMS {err:.3e}"
            if epi and k > 2048 and not pro:      # the atomic form: K slices, a linear epilogue, no prologue, res == out
                lib.vv_tune(b"gemv_rows_atomic", 1)
                out2 = res.clone()
                a = args(True, out2)
                a.res = out2.data_ptr()
                L.check(lib.vv_linear_route(C.byref(a), name, 192), "vv_linear_route")
                assert name.value.decode().endswith("atomic=1"), name.value
                L.check(lib.vv_linear(C.byref(a), s), "vv_linear atomic")
                torch.cuda.synchronize()
                err = rel_rms(out2.double().cpu().numpy(), y.cpu().numpy())
                print(f"{case} m={m}: in place (atomic) vs fp64 rel RMS {err:.3e}")
                assert err < 2e-5, f"mxfp4 rows GEMV in place (atomic) {case} m={m}: rel RMS {err:.3e}"
    finally:
        lib.vv_tune(b"gemv_rows_scratch", 0)


# ---------------------------------------------------------------------------------------------------------------
# 2. refusals
# ---------------------------------------------------------------------------------------------------------------
def test_refusals(lib):
    """m <= 2, m > 8, a missing scale pointer (of w, of w2), a misaligned pointer (codes, scales), VV_LIN_X_BF16 / VV_LIN_OUT_BF16, the flag
    missing, n % 16, k % 128: VV_E_UNSUPPORTED from vv_linear_route and from vv_linear alike, the output untouched; the same call without the
    fault runs.  VV_MXFP4 keeps refusing the flag and 3 rows."""
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.weights import DeviceWeights, quantize_mxfp4
    n, k = 64, 1024
    c, s, _ = quantize_mxfp4(torch.randn(n, k))
    f = DeviceWeights.frag_major_mxfp4(c, s)
    f = torch.cat([f, f]).cuda()                                         # room behind every offset pointer below
    p, q = f.data_ptr(), f.data_ptr() + n * k // 2
    x = torch.randn(12, k, device="cuda")
    out = torch.full((12, n), float("nan"), device="cuda")
    name = C.create_string_buffer(192)

    def args(m=4, nn=n, kk=k, flags=L.LIN_W_FRAG, wdt=L.VV_MXFP4_FRAG, **kw):
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
               "n%16": args(nn=56), "k%128": args(kk=k - 64), "mxfp4 + flag, 4 rows": args(wdt=L.VV_MXFP4), "mxfp4, 3 rows": args(3, flags=0, wdt=L.VV_MXFP4)}
    for what, a in refused.items():
        rc_route = lib.vv_linear_route(C.byref(a), name, 192)
        rc_run = lib.vv_linear(C.byref(a), None)
        assert rc_route == rc_run == VV_E_UNSUPPORTED, (what, rc_route, rc_run, lib.vv_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its output"
    for a in (args(), args(3), args(8, **dual)):
        assert lib.vv_linear_route(C.byref(a), name, 192) == 0 and name.value.decode().startswith("gemv_rows_mx<"), lib.vv_last_error()
        assert lib.vv_linear(C.byref(a), None) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out[:8]).all() and torch.isnan(out[8:]).all()
    # beyond K = 2048 the K slices need scratch (or the in-place atomic form): refused without, the output untouched
    k2 = 4096
    c, s, _ = quantize_mxfp4(torch.randn(n, k2))
    f2 = DeviceWeights.frag_major_mxfp4(c, s).cuda()
    x2 = torch.randn(4, k2, device="cuda")
    out.fill_(float("nan"))
    a = args(kk=k2, x=x2.data_ptr(), ldx=k2, w=f2.data_ptr(), wscale=f2.data_ptr() + n * k2 // 2)
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
                                                                  weight_quant="mxfp4", **kw)
    m.set_ddpm_inference_steps(N_STEPS)
    return cfg, m


@pytest.fixture(scope="module")
def mid():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _mid_model(mxfp4_row_batch=True)


def _companion_shapes(cfg):
    """(n, k) of every matrix that has an MXFP4 companion on the LLM and head path, by f_* name"""
    qkvd, hd = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, cfg.heads * cfg.head_dim
    llm = {"qkv": (qkvd, cfg.hidden), "o": (cfg.hidden, hd), "gate": (cfg.inter, cfg.hidden), "up": (cfg.inter, cfg.hidden), "down": (cfg.hidden, cfg.inter)}
    head = {"gate": (cfg.head_ffn, cfg.head_hidden), "up": (cfg.head_ffn, cfg.head_hidden), "down": (cfg.head_hidden, cfg.head_ffn)}
    return llm, head


def _mx_frag_ptrs(w):
    """every f_* pointer of the LLM and head layers: a uint8 VV_MXFP4_FRAG copy (codes + scale bytes) where the shape fits, NULL elsewhere - and
    for the head's gate / up pair beyond K = 2048, which no MX rows route takes with its adaLN prologue (7B widths): no copy that is never read"""
    by_ptr = {t.data_ptr(): t for t in w._frag_state["tensors"]}
    llm, head = _companion_shapes(w.cfg)
    ptrs = []
    for lay, shapes in [(w.llm.layer[l], llm) for l in range(w.cfg.layers)] + [(w.head.layer[l], head) for l in range(w.cfg.head_layers)]:
        for nm, (n, k) in shapes.items():
            p = getattr(lay, "f_" + nm)
            if n % 16 or k % 128 or (shapes is head and nm in ("gate", "up") and k > 2048):
                assert not p
                continue
            assert p and by_ptr[p].dtype == torch.uint8 and by_ptr[p].numel() == n * k // 2 + n * k // 32, f"f_{nm}"
            ptrs.append(p)
    assert all(t.dtype == torch.uint8 for t in w._frag_state["tensors"]), "a bf16 fragment copy next to the MXFP4 ones"
    return ptrs


def test_decode_step_8_rows_mxfp4_vs_batch2(mid):
    """One row-batched MXFP4 decode step (8 rows on the fragment-major codes) against the MXFP4 batch-2 step (1..2-row streaming GEMV) of every
    dialogue on its own engine state: hidden rows, constrained logits, tokens, positions.  Bars of test_decode_step_8_rows_fp8_vs_batch2."""
    _decode_step_vs_batch2(*mid, "mid")


def _decode_step_vs_batch2(cfg, m, tag):
    from vibevoice_rocm_amd.rowbatch import RowBatch
    tok = _Tok(cfg.vocab)
    ST, SD = tok.speech_start_id, tok.speech_diffusion_id
    valid = [ST, tok.speech_end_id, SD, tok.eos_token_id]
    B = 4
    lanes = [m._lane(b) for b in range(B)]
    rb = RowBatch(lanes)
    _mx_frag_ptrs(m.engine.w)
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
                     what=f"row-batched mxfp4 decode step {tag}, dialogue {b} of 4: hidden rows vs the mxfp4 batch-2 step")
        el = rel_rms(rb.logits[b, :4].cpu().numpy(), ref_logits[b].cpu().numpy())
        print(f"{tag} dialogue {b}: hidden {eh:.3e} logits {el:.3e}")
        assert eh < 5e-3 and el < 5e-3, f"dialogue {b}: hidden {eh:.3e} logits {el:.3e}"
        assert toks[b] == ref_tok[b]
        assert rb.lens[2 * b: 2 * b + 2].tolist() == ref_lens[b].tolist()
    rb.close()


@pytest.mark.parametrize("solver", ["ode", "sde"])
def test_head_sample_batch_mxfp4_vs_single(mid, solver):
    """The batched head sampler (4 utterances, 8 rows per pass over the MXFP4 fragment-major codes) against the MXFP4 single-utterance sampler,
    under the ODE and the SDE solver.  Bar of test_head_sample_batch_fp8_vs_single."""
    cfg, m = mid
    eng = m.engine
    lb = eng.lib
    eng.w.ensure_frag()
    _mx_frag_ptrs(eng.w)
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
                          what=f"row-batched mxfp4 head sampling ({solver}) mid, utterance {b} of 4, vs the mxfp4 single-utterance sampler")
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
    return ids, mask


def test_generate_mxfp4_row_batch_vs_lanes(mid):
    """generate() on 3 dialogues with different token schedules (an early end, a turn switch): the opt-in takes the row batch, row_batch=False keeps
    the lanes; same sequences, waveforms at the bar of test_generate_fp8_row_batch_vs_lanes."""
    cfg, m = mid
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(64)
    ids, mask = _padded(tok, [40, 31, 36], g)
    forced = [[D] * 5 + [E, EOS], [D] * 3 + [E, S, D, D, E, EOS], [D] * 2 + [E, EOS]]
    noise = torch.randn(3, 8, cfg.latent, generator=g)
    kw = dict(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    m.release_lanes()
    lanes = m.generate(row_batch=False, **kw)
    assert not m._rowbatch, "row_batch=False took the row-batched path"
    rows = m.generate(**kw)
    assert (3, 0) in m._rowbatch, "mxfp4_row_batch=True on 3 dialogues did not take the row-batched path"
    _mx_frag_ptrs(m.engine.w)
    assert rows.sequences.tolist() == lanes.sequences.tolist()
    for b in range(3):
        a, r = rows.speech_outputs[b], lanes.speech_outputs[b]
        assert a.shape == r.shape
        err = rel_rms(a.float().cpu().numpy(), r.float().cpu().numpy(), what=f"generate() mxfp4 on 3 dialogues mid, row-batched vs lanes, waveform of dialogue {b}")
        print(f"dialogue {b}: row-batched vs lanes {err:.3e}")
        assert err < 1e-2, f"dialogue {b}: waveform rel RMS {err:.3e}"


def test_generate_mxfp4_row_batch_mid_vs_oracle(mid):
    """The row-batched call on 3 dialogues (4 voice prompts each, turn switches) against the CPU oracle on mxfp4_effective_state_dict under
    2e-2, the single-dialogue MXFP4 bar; the bf16 model, row-batched on the same call, is further than that bar from it - the test would not
    pass on unquantised weights."""
    from oracle import vv_oracle as O
    from test_hip_configs import _four_speaker_inputs, _special
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict
    from vibevoice_rocm_amd.weights import fp8_matrix_names, mxfp4_effective_state_dict
    cfg, m = mid
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, MID_SEED).items()}
    eff = mxfp4_effective_state_dict(cfg, sd)
    names = set(fp8_matrix_names(cfg))
    sd_o = {k: (eff[k] if k in names else (v.to(torch.bfloat16).float() if v.dim() >= 2 else v)) for k, v in sd.items()}
    V = cfg.vocab
    ST, SE, SD, EOS = V - 4, V - 3, V - 2, V - 1
    g = torch.Generator().manual_seed(29)
    ids, sp_mask, wav, sm = _four_speaker_inputs(cfg, g)
    forced = [([SD] * 4 + [SE, ST]) * 2 + [SD] * 4 + [SE, EOS], [SD] * 7 + [SE, ST] + [SD] * 3 + [SE, EOS], [SD] * 5 + [SE, EOS]]
    noise = torch.randn(3, 12, cfg.latent, generator=g)
    std_noise, eps_noise = torch.randn(4, generator=g), torch.randn(4, 4, cfg.ac_dim, generator=g)
    _, conn = O.process_speech_inputs(sd_o, cfg.as_dict(), wav, sm, std_noise, eps_noise)
    refs = [O.generate(sd_o, cfg.as_dict(), ids.tolist(), sp_mask, conn, _special(V), noise[b], cfg_scale=2.0, n_steps=N_STEPS, forced_tokens=forced[b], bf16_t=True)
            for b in range(3)]
    tok = _Tok(V, pad=0)
    kw = dict(input_ids=ids[None].repeat(3, 1), attention_mask=torch.ones(3, ids.shape[0], dtype=torch.long), speech_tensors=wav.repeat(3, 1), speech_masks=sm.repeat(3, 1),
              speech_input_mask=sp_mask[None].repeat(3, 1), tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise,
              speech_noise=(std_noise.repeat(3), eps_noise.repeat(3, 1, 1)))
    m.release_lanes()
    out = m.generate(**kw)
    assert (3, 0) in m._rowbatch
    m16 = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m16.set_ddpm_inference_steps(N_STEPS)
    out16 = m16.generate(**kw)
    assert (3, 0) in m16._rowbatch
    for b in range(3):
        want = torch.cat(refs[b].audio).numpy()
        assert out.sequences[b, ids.shape[0]: ids.shape[0] + len(forced[b])].tolist() == forced[b]
        got = out.speech_outputs[b][0].float().cpu().numpy()
        err = rel_rms(got, want, what=f"generate() 3 dialogues, mid mxfp4, ROW-BATCHED vs oracle on the effective weights, dialogue {b}")
        far = rel_rms(out16.speech_outputs[b][0].float().cpu().numpy(), got)
        print(f"dialogue {b}: mxfp4 row-batched vs oracle {err:.3e}; bf16 row-batched vs mxfp4 row-batched {far:.3e}")
        assert err < 2e-2, f"row-batched mxfp4 dialogue {b}: waveform rel RMS {err:.3e} vs oracle"
        assert far > 2e-2, f"dialogue {b}: the bf16 model is within the bar of the mxfp4 one ({far:.3e}): the test would pass on unquantised weights"
    m16.release_lanes()          # its engines end here: their HIP streams go back to the recycle pool for the tests that follow
    del m16, out16
    gc.collect()
    torch.cuda.empty_cache()


def test_row_batch_streams_mxfp4_frag_for_every_companion_matrix():
    """Under vv_prof_begin / vv_prof_end an eager row-batched generate() on 3 dialogues (6 rows) records, for every matrix that has a companion
    and K % 128 == 0, launches with wdt == VV_MXFP4_FRAG at 3 <= m <= 8 - once per layer per decode step, once per head layer per solver step per
    sampler call at least - and no bf16 launch of that matrix in that row range.  At `mid` the o projection shares its shape [512, 512] with the
    head's cond_proj (no companion: bf16, once per sampler call): its bf16 count must be exactly the number of sampler calls, which the other
    records give."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    lb = L.load()
    cfg, m = _mid_model(mxfp4_row_batch=True, use_graphs=False)
    steps = 10
    m.set_ddpm_inference_steps(steps)
    tok = _Tok(cfg.vocab)
    D, E, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id
    g = torch.Generator().manual_seed(16)
    ids, mask = _padded(tok, [24, 20, 22], g)
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
    assert all(3 <= e.m <= 8 for e in rec if e.wdt == L.VV_MXFP4_FRAG)
    mx = {}
    for e in rec:
        if e.wdt == L.VV_MXFP4_FRAG:
            assert e.m == 6
            mx[(e.n, e.k, e.dual)] = mx.get((e.n, e.k, e.dual), 0) + e.count
    bf = {}
    for e in rec:
        if e.wdt == L.VV_BF16 and 3 <= e.m <= 8:
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
        assert mx.get(key, 0) >= least, f"{key}: {mx.get(key, 0)} VV_MXFP4_FRAG launches at 6 rows, expected at least {least}"
    assert llm["gate"] == head["gate"] and llm["o"] == (cfg.head_hidden, cfg.hidden), "the shape bookkeeping below is for `mid`"
    steps_a = mx[(*llm["qkv"], 0)] // cfg.layers                                          # row-batched decode steps
    calls_h = (mx[(*llm["gate"], 1)] - cfg.layers * steps_a) // (cfg.head_layers * steps)  # batched sampler calls
    assert steps_a >= decodes and calls_h >= frames
    for key in want:
        if key == (*llm["o"], 0):
            assert bf.get(key, 0) == calls_h, f"{key}: {bf.get(key, 0)} bf16 launches at 3..8 rows, the head's cond_proj accounts for {calls_h}"
        else:
            assert bf.get(key, 0) == 0, f"{key}: {bf[key]} bf16 launches at 3..8 rows next to the MXFP4 fragment copies"
    m.release_lanes()
    del m
    gc.collect()
    torch.cuda.empty_cache()


def test_fragment_copies_are_built_once(mid):
    """A 3-dialogue call, then a 6-dialogue call (two row batches, the second led by a forked lane): the MXFP4 fragment copies are built once
    for the weights and every fork; the VRAM record is 0.53125 bytes per copied weight, as nbytes() counts it."""
    cfg, m = mid
    tok = _Tok(cfg.vocab)
    D, E, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.eos_token_id
    g = torch.Generator().manual_seed(3)
    m.set_ddpm_inference_steps(10)

    def call(B):
        ids, mask = _padded(tok, [20 + b for b in range(B)], g)
        m.generate(input_ids=ids, attention_mask=mask, tokenizer=tok, cfg_scale=2.0, forced_tokens=[[D, D, E, EOS]] * B,
                   noise=torch.randn(B, 4, cfg.latent, generator=g))

    try:
        m.release_lanes()
        call(3)
        assert (3, 0) in m._rowbatch
        w = m.engine.w
        ptrs = _mx_frag_ptrs(w)
        n_frag = len(w._frag_state["tensors"])
        call(6)
        assert len(m._rowbatch) >= 2
        torch.cuda.synchronize()
        assert _mx_frag_ptrs(w) == ptrs and len(w._frag_state["tensors"]) == n_frag
        mem = torch.cuda.memory_allocated()
        for e in m._lanes:
            e.w.ensure_frag()
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == mem, "a forked lane built its own fragment copies"
        llm, head = _companion_shapes(cfg)
        weights = cfg.layers * sum(n * k for n, k in llm.values()) + cfg.head_layers * sum(n * k for n, k in head.values())
        st = w._frag_state
        assert st["mxfp4_weights"] == weights and st["mxfp4_bytes"] == weights * 17 // 32 == sum(t.numel() for t in st["tensors"])
    finally:
        m.set_ddpm_inference_steps(N_STEPS)


# ---------------------------------------------------------------------------------------------------------------
# 4. a session
# ---------------------------------------------------------------------------------------------------------------
def test_session_mxfp4_vs_generate_alone(mid):
    """open_session on the opt-in model: three requests of different lengths through two slots - the third is admitted into a reused slot - each
    against generate() on it alone (the single-dialogue MXFP4 engine) at the bar of test_session_vs_each_dialogue_alone (1e-2).  A model
    without the keyword still raises the parent's error."""
    cfg, m = mid
    tok = _Tok(cfg.vocab)
    D, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(61)
    lens, scales = [44, 30, 37], [1.3, 2.0, 3.0]
    prompts = [torch.cat([torch.randint(0, 1000, (n - 1,), generator=g), torch.tensor([S])]) for n in lens]
    forced = [[D] * 6 + [E, EOS], [D] * 2 + [E, EOS], [D] * 3 + [E, S] + [D] * 2 + [E, EOS]]
    noise = torch.randn(3, 8, cfg.latent, generator=g)
    m.release_lanes()
    with m.open_session(tokenizer=tok, slots=2, max_context=256, device_noise=False) as sess:
        hs = [sess.submit(input_ids=prompts[i][None], cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i]) for i in range(3)]
        sess.run()
    assert m._session is None and all(h.done for h in hs)
    assert [h.slot for h in hs] == [0, 1, 1], "the third request takes over the slot of the one that ended first"
    _mx_frag_ptrs(m.engine.w)
    for i in range(3):
        want = m.generate(input_ids=prompts[i][None], tokenizer=tok, cfg_scale=scales[i], forced_tokens=forced[i], noise=noise[i])
        got = hs[i].result()
        assert got.sequences.tolist() == want.sequences.tolist() == [prompts[i].tolist() + forced[i]]
        err = rel_rms(got.speech_outputs[0].float().cpu().numpy(), want.speech_outputs[0].float().cpu().numpy(),
                      what=f"session of 2 slots, mid mxfp4, dialogue {i} (cfg {scales[i]}, slot {hs[i].slot}) vs generate() alone")
        print(f"session dialogue {i} slot {hs[i].slot}: waveform rel RMS {err:.3e}")
        assert err < 1e-2, f"dialogue {i}: waveform rel RMS {err:.3e}"
    _, plain = _mid_model()
    assert not plain.mxfp4_row_batch and plain.engine.w.llm.wdt & 0x400 == 0
    with pytest.raises(ValueError, match="weight_quant='mxfp4'"):
        plain.open_session(tokenizer=tok, max_context=256)
    del plain
    gc.collect()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------
# 5. the 7B widths
# ---------------------------------------------------------------------------------------------------------------
def test_decode_step_8_rows_mxfp4_7b_widths_vs_batch2():
    """7B widths (H 3584, I 18944; 2 LLM layers): the 8-row step - qkv / o on 3-slice K splits, the SwiGLU pair on a 2-slice split, the down
    projection on 13 slices folded through tickets or added in place - against the batch-2 MXFP4 step, GPU against GPU."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = dataclasses.replace(VVConfig.preset("7b"), layers=2)
    sd = synth_state_dict_torch(cfg, 778, device="cuda:0", dtype=torch.bfloat16)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="mxfp4", mxfp4_row_batch=True)
    del sd
    try:
        _decode_step_vs_batch2(cfg, m, "7B widths")
    finally:
        m.release_lanes()
        del m
        gc.collect()
        torch.cuda.empty_cache()
