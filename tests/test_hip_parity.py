"""GPU parity tests: the HIP path (through the C ABI) against
  (1) the golden fixtures captured from the reference's own modules (tiny shapes, weights from the numpy generator),
  (2) the CPU oracle on seeded inputs at `mid` shapes (real head_dim / GQA, vectorised kernel paths),
  (3) a plain torch fp32 reference for the fused linear primitive over the shape/alignment/prologue/epilogue matrix.
Tolerance: fp32 weights, relative RMS <= 1e-4 per component (north_star bar: waveform RMS <= 1e-3);
bf16 weights are compared with the oracle run on the same bf16-rounded weights, <= 5e-3.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_rms, vt_tiles

pytestmark = pytest.mark.gpu

F32_TOL = 1e-4


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def lib():
    _need_gpu()
    from vibevoice_rocm_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def tiny_engine(tiny_cfg, tiny_weights):
    _need_gpu()
    from vibevoice_rocm_amd.engine import Engine
    return Engine(tiny_cfg, tiny_weights, device="cuda:0", dtype=torch.float32, use_graphs=False)


def dev(x):
    return torch.as_tensor(np.asarray(x)).to("cuda:0")


# ---------------------------------------------------------------------------------------------------------------
# (3) fused linear primitive vs torch
# ---------------------------------------------------------------------------------------------------------------
def _ref_linear(x, w, w2, bias, pro, norm_w, eps, shift, scale, act, gate, res):
    x = x.double()
    if pro == 1:
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)
        if norm_w is not None:
            x = x * norm_w.double()
        if scale is not None:
            x = x * (1 + scale.double()) + shift.double()
    elif pro == 2:
        x = x * torch.sigmoid(x)
    y = x @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    if act == 1:
        y = torch.nn.functional.gelu(y)
    elif act == 2:
        y = (y * torch.sigmoid(y)) * (x @ w2.double().t())
    if gate is not None:
        y = y * gate.double()
    if res is not None:
        y = y + res.double()
    return y


@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("m,n,k", [(1, 1536, 1536), (2, 8960, 1536), (2, 1536, 8960), (2, 64, 1536), (1, 2048, 448),
                                   (8, 4096, 1024), (2, 37, 14), (3, 5, 64), (40, 4608, 1536), (200, 1024, 256),
                                   (3200, 128, 32), (33, 70, 56), (100, 1, 224), (17, 9, 7),
                                   (2, 3584, 10752), (2, 512, 18944), (1, 256, 24576), (4, 1024, 4096), (7, 640, 2048),
                                   (8, 1024, 4096), (8, 1024, 5120), (6, 2560, 2048), (5, 96, 512), (8, 64, 16384)])
def test_linear_shapes(lib, m, n, k, wdtype):
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(m * 1000 + n + k)
    x = torch.randn(m, k, generator=g)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(wdtype)
    bias = torch.randn(n, generator=g) * 0.1
    res = torch.randn(m, n, generator=g)
    xd, wd, bd, rd = x.cuda(), w.cuda(), bias.cuda(), res.cuda()
    out = torch.zeros(m, n, device="cuda")
    a = L.LinArgs()
    a.x, a.ldx, a.m = xd.data_ptr(), k, m
    a.w, a.n, a.k, a.wdt = wd.data_ptr(), n, k, (L.VV_F32 if wdtype == torch.float32 else L.VV_BF16)
    a.bias = bd.data_ptr()
    a.res, a.ldres = rd.data_ptr(), n
    a.out, a.ldo = out.data_ptr(), n
    L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    ref = _ref_linear(x, w.float(), None, bias, 0, None, 0, None, None, 0, None, res)
    # bf16 weights with more than 8 rows run on the matrix cores with activations rounded to bf16 at staging
    tol = 4e-3 if (wdtype == torch.bfloat16 and m > 8) else 2e-6
    assert rel_rms(out.cpu().numpy(), ref.numpy()) < tol


@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("m,n,k", [(2, 192, 128), (24, 192, 128), (2, 256, 3584), (2, 320, 1536), (8, 256, 1024), (7, 128, 4096)])
@pytest.mark.parametrize("variant", ["rms_swiglu", "rms_mod_gate", "silu", "gelu_gamma", "rms_noaffine"])
def test_linear_fusions(lib, m, n, k, variant, wdtype):
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(7)
    x = torch.randn(m, k, generator=g)
    w = (torch.randn(n, k, generator=g) / k ** 0.5).to(wdtype)
    w2 = (torch.randn(n, k, generator=g) / k ** 0.5).to(wdtype)
    norm_w = 1 + 0.1 * torch.randn(k, generator=g)
    shift = 0.2 * torch.randn(m, k, generator=g)
    scale = 0.2 * torch.randn(m, k, generator=g)
    gate_row = torch.randn(m, n, generator=g)
    gamma = torch.randn(n, generator=g)
    bias = torch.randn(n, generator=g)
    res = torch.randn(m, n, generator=g)
    t = {kk: v.cuda() for kk, v in dict(x=x, w=w, w2=w2, norm_w=norm_w, shift=shift, scale=scale, gate_row=gate_row, gamma=gamma, bias=bias, res=res).items()}
    out = torch.zeros(m, n, device="cuda")
    a = L.LinArgs()
    a.x, a.ldx, a.m = t["x"].data_ptr(), k, m
    a.w, a.n, a.k, a.wdt = t["w"].data_ptr(), n, k, (L.VV_F32 if wdtype == torch.float32 else L.VV_BF16)
    a.out, a.ldo = out.data_ptr(), n
    a.eps = 1e-5
    w, w2 = w.float(), w2.float()
    kw = dict(w2=None, bias=None, pro=0, norm_w=None, eps=1e-5, shift=None, scale=None, act=0, gate=None, res=None)
    if variant == "rms_swiglu":
        a.pro, a.norm_w, a.w2, a.act = 1, t["norm_w"].data_ptr(), t["w2"].data_ptr(), 2
        kw.update(pro=1, norm_w=norm_w, w2=w2, act=2)
    elif variant == "rms_mod_gate":
        a.pro, a.norm_w = 1, t["norm_w"].data_ptr()
        a.mod_shift, a.mod_scale, a.ld_mod = t["shift"].data_ptr(), t["scale"].data_ptr(), k
        a.gate, a.gate_ld, a.res, a.ldres = t["gate_row"].data_ptr(), n, t["res"].data_ptr(), n
        kw.update(pro=1, norm_w=norm_w, shift=shift, scale=scale, gate=gate_row, res=res)
    elif variant == "silu":
        a.pro = 2
        kw.update(pro=2)
    elif variant == "gelu_gamma":
        a.bias, a.act, a.gate, a.gate_ld, a.res, a.ldres = t["bias"].data_ptr(), 1, t["gamma"].data_ptr(), 0, t["res"].data_ptr(), n
        kw.update(bias=bias, act=1, gate=gamma, res=res)
    elif variant == "rms_noaffine":
        a.pro = 1
        a.mod_shift, a.mod_scale, a.ld_mod = t["shift"].data_ptr(), t["scale"].data_ptr(), k
        kw.update(pro=1, shift=shift, scale=scale)
    L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    ref = _ref_linear(x, w, w2 if kw["w2"] is not None else None, kw["bias"], kw["pro"], kw["norm_w"], kw["eps"], kw["shift"], kw["scale"], kw["act"], kw["gate"], kw["res"])
    tol = 5e-3 if (wdtype == torch.bfloat16 and m > 8) else 4e-6
    assert rel_rms(out.cpu().numpy(), ref.numpy()) < tol


def test_dpm_step_and_fused_boundary_agree(lib):
    """vv_dpm_step (stand-alone CFG + DPM-Solver++ update) and vv_dpm_proj (the same update fused with noisy_images_proj) against
    the closed form, first and second order."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(3)
    latent, D = 64, 96
    v = torch.randn(2, latent, generator=g); x = torch.randn(latent, generator=g); mp = torch.randn(latent, generator=g)
    W = torch.randn(D, latent, generator=g) / 8
    for order in (1, 2):
        c = L.DpmCoef(); c.alpha_s, c.sigma_s, c.cx, c.cd, c.rinv, c.order = 0.7, 0.6, 0.9, -0.3, 1.7, order
        eps = v[1] + 2.0 * (v[0] - v[1])
        x0 = 0.7 * x - 0.6 * eps
        ref = 0.9 * x - (-0.3) * x0 - (0.5 * (-0.3) * (1.7 * (x0 - mp)) if order == 2 else 0)
        vd, xd, md = v.cuda(), x.cuda().clone(), mp.cuda().clone()
        L.check(l.vv_dpm_step(vd.data_ptr(), latent, 1, latent, 2.0, 0.7, 0.6, 0.9, -0.3, 1.7, order, xd.data_ptr(), md.data_ptr(), None), "dpm_step")
        xo, mo, h = torch.zeros(latent, device="cuda"), torch.zeros(latent, device="cuda"), torch.zeros(2, D, device="cuda")
        Wd, xi, mi = W.cuda(), x.cuda(), mp.cuda()
        L.check(l.vv_dpm_proj(vd.data_ptr(), latent, 2.0, C.byref(c), xi.data_ptr(), mi.data_ptr(), xo.data_ptr(), mo.data_ptr(),
                              Wd.data_ptr(), L.VV_F32, latent, D, h.data_ptr(), D, 2, None, None), "dpm_proj")
        torch.cuda.synchronize()
        assert rel_rms(xd.cpu().numpy(), ref.numpy()) < 1e-6 and rel_rms(xo.cpu().numpy(), ref.numpy()) < 1e-6
        assert rel_rms(md.cpu().numpy(), x0.numpy()) < 1e-6 and rel_rms(mo.cpu().numpy(), x0.numpy()) < 1e-6
        assert rel_rms(h[1].cpu().numpy(), (W @ ref).numpy()) < 1e-5 and torch.equal(h[0], h[1])


@pytest.mark.parametrize("T,C_", [(1, 2048), (8, 1024), (40, 512), (200, 256), (3, 256), (9, 512), (17, 1024), (256, 256), (300, 256), (5, 96)])
def test_block_mixer_vs_torch(lib, T, C_):
    """vv_block_mixer: x + gamma * (dwconv7_causal(RMSNorm(x)) + b), three consecutive streaming calls (history carried) and a
    stateless call, against torch fp32.  Covers the few-rows kernel (T <= 256, C in 256..2048) and the sliced kernel (the rest)."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(1000 + T + C_)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    nw, dw, db, gm = 1 + r(C_, sc=0.1), r(C_, 7, sc=0.3), r(C_, sc=0.1), r(C_, sc=0.5)
    eps = 1e-5
    d = [t.cuda().contiguous() for t in (nw, dw, db, gm)]
    hist_dev = torch.zeros(6, C_, device="cuda")
    hist = torch.zeros(6, C_)
    for call in range(4):
        x = r(T, C_)
        streaming = call < 3
        xn = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * nw
        seq = torch.cat([hist if streaming else torch.zeros(6, C_), xn])
        want = x + gm * (db + sum(dw[:, k] * seq[k: k + T] for k in range(7)))
        xd, od = x.cuda(), torch.full((T, C_), float("nan"), device="cuda")
        L.check(l.vv_block_mixer(xd.data_ptr(), od.data_ptr(), T, C_, d[0].data_ptr(), eps, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(),
                                 hist_dev.data_ptr() if streaming else None, None), "vv_block_mixer")
        torch.cuda.synchronize()
        assert rel_rms(od.cpu().numpy(), want.numpy()) < 2e-6, (call, T, C_)
        if streaming:
            hist = seq[-6:]
            assert rel_rms(hist_dev.cpu().numpy(), hist.numpy()) < 2e-6, (call, T, C_)


@pytest.mark.parametrize("C_", [32, 64, 128])
@pytest.mark.parametrize("T", [32, 45, 800])
def test_block1d_single_launch_vs_torch(lib, C_, T):
    """vv_block1d (mixer + FFN of one Block1D in one launch, bf16 weights on the matrix cores) against a torch fp32 restatement
    of Block1D.forward (modular_vibevoice_tokenizer.py:555-600) on the same bf16-rounded weights; two consecutive streaming calls
    (history carried in b.hist) and a stateless call.  Tolerance: activations are rounded to bf16 at the two GEMM inputs."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(100 + C_ + T)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    p = dict(gamma=r(C_, sc=0.5), ffn_gamma=r(C_, sc=0.5), norm_w=1 + r(C_, sc=0.1), ffn_norm_w=1 + r(C_, sc=0.1), dw_w=r(C_, 7, sc=0.3), dw_b=r(C_, sc=0.1),
             w1=(r(4 * C_, C_) / C_ ** 0.5).bfloat16(), b1=r(4 * C_, sc=0.1), w2=(r(C_, 4 * C_) / (4 * C_) ** 0.5).bfloat16(), b2=r(C_, sc=0.1))
    eps = 1e-5

    def rms(x, w): return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w

    def ref(x, hist):
        xn = rms(x, p["norm_w"])
        seq = torch.cat([hist, xn])
        s = p["dw_b"] + sum(p["dw_w"][:, k] * seq[k: k + x.shape[0]] for k in range(7))
        x1 = x + p["gamma"] * s
        h = torch.nn.functional.gelu(rms(x1, p["ffn_norm_w"]) @ p["w1"].float().T + p["b1"])
        return x1 + p["ffn_gamma"] * (h @ p["w2"].float().T + p["b2"]), seq[-6:]

    d = {k: v.cuda().contiguous() for k, v in p.items()}
    hist_dev = torch.zeros(6, C_, device="cuda")
    b = L.Block()
    for k in ("gamma", "ffn_gamma", "norm_w", "ffn_norm_w", "dw_w", "dw_b", "w1", "b1", "w2", "b2"):
        setattr(b, k, d[k].data_ptr())
    hist = torch.zeros(6, C_)
    for call in range(3):                       # calls 0, 1: streaming; call 2: stateless (zero left context)
        x = r(T, C_)
        streaming = call < 2
        b.hist = hist_dev.data_ptr() if streaming else None
        want, new_hist = ref(x, hist if streaming else torch.zeros(6, C_))
        xd, od = x.cuda(), torch.full((T, C_), float("nan"), device="cuda")
        L.check(l.vv_block1d(C.byref(b), L.VV_BF16, xd.data_ptr(), od.data_ptr(), T, C_, eps, None), "vv_block1d")
        torch.cuda.synchronize()
        assert rel_rms(od.cpu().numpy(), want.numpy()) < 1e-2, (call, C_, T)
        if streaming:
            hist = new_hist
            assert rel_rms(hist_dev.cpu().numpy(), hist.numpy()) < 1e-5, (call, C_, T)
    # not covered -> explicit refusal, never a silent fallback
    assert l.vv_block1d(C.byref(b), L.VV_F32, xd.data_ptr(), od.data_ptr(), T, C_, eps, None) != 0
    assert l.vv_block1d(C.byref(b), L.VV_BF16, xd.data_ptr(), od.data_ptr(), 8, C_, eps, None) != 0


@pytest.mark.parametrize("m,n,k,dual,pro,mod,epi,act", [
    (2, 4608, 1536, True, 1, True, False, 2), (2, 1536, 4608, False, 0, False, True, 0), (2, 8960, 1536, True, 1, False, False, 2),
    (2, 1536, 8960, False, 0, False, True, 0), (2, 2048, 1536, False, 1, False, False, 0), (2, 1536, 1536, False, 0, False, True, 0),
    (1, 8192, 2048, False, 1, False, False, 1), (1, 2048, 8192, False, 0, False, True, 0), (4, 4608, 1536, True, 1, True, False, 2),
    (3, 1536, 4608, False, 0, False, True, 0), (2, 10752, 3584, True, 1, True, False, 2), (2, 3584, 3584, False, 1, False, False, 0),
    (1, 64, 1536, False, 1, True, False, 0), (2, 132, 1536, False, 0, False, False, 0)])
def test_decode_gemv_vs_torch(lib, m, n, k, dual, pro, mod, epi, act):
    """vv_linear at the decode shapes (1..4 rows, bf16 weights) on the weight-streaming GEMV against torch fp64 on the bf16-rounded weights:
    RMSNorm / adaLN-modulate prologues, bias, GELU, SwiGLU, per-row gate and residual epilogues, K split over waves (k > 2048) and whole-row waves."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(m * 7 + n + k)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    x = r(m, k)
    w = (r(n, k) / k ** 0.5).bfloat16()
    w2 = (r(n, k) / k ** 0.5).bfloat16()
    nw, sh, sc = 1 + r(k, sc=0.1), r(m, k, sc=0.2), r(m, k, sc=0.2)
    bias, gate, res = r(n, sc=0.1), r(m, n, sc=0.5), r(m, n)
    d = [t.cuda().contiguous() for t in (x, w, w2, nw, sh, sc, bias, gate, res)]
    out = torch.full((m, n), float("nan"), device="cuda")
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo = d[0].data_ptr(), k, m, n, k, L.VV_BF16, out.data_ptr(), n
    a.w = d[1].data_ptr()
    xp = x
    if pro == 1:
        a.pro, a.norm_w, a.eps = 1, d[3].data_ptr(), 1e-5
        xp = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-5) * nw
        if mod:
            a.mod_shift, a.mod_scale, a.ld_mod = d[4].data_ptr(), d[5].data_ptr(), k
            xp = xp * (1 + sc) + sh
    y = xp.double() @ w.double().T
    if dual:
        a.w2, a.act = d[2].data_ptr(), 2
        y = torch.nn.functional.silu(y) * (xp.double() @ w2.double().T)
    elif act == 1:
        a.bias, a.act = d[6].data_ptr(), 1
        y = torch.nn.functional.gelu(y + bias.double())
    if epi:
        a.gate, a.gate_ld, a.res, a.ldres = d[7].data_ptr(), n, d[8].data_ptr(), n
        y = y * gate.double() + res.double()
    L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    e = rel_rms(out.cpu().numpy(), y.float().numpy())
    assert e < 2e-5, f"m={m} n={n} k={k} dual={dual} pro={pro} mod={mod} epi={epi} act={act}: rel RMS {e:.3e}"


@pytest.mark.parametrize("m,n,k,ldx", [(40, 512, 2560, 1280), (200, 256, 1024, 512), (40, 1280, 1024, 1024), (200, 512, 512, 512), (8, 2560, 2048, 2048),
                                       (37, 48, 2560, 2564), (5, 16, 512, 512), (256, 1024, 1024, 1028), (8, 1024, 5120, 2560), (800, 128, 256, 128), (1600, 64, 128, 64), (1603, 32, 128, 132)])
def test_resampling_conv_skinny_gemm_vs_torch(lib, m, n, k, ldx):
    """vv_linear at the shapes of a streaming frame's resampling convs (fp32 rows with overlapping windows: ldx < k for a strided conv,
    bf16 weights, bias, no activation): the LDS-free skinny kernel of vv_convffn.hip against torch on the bf16-rounded operands."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(m + n + k)
    buf = torch.randn((m - 1) * ldx + k, generator=g)
    x = torch.stack([buf[i * ldx: i * ldx + k] for i in range(m)])
    w = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
    bias = torch.randn(n, generator=g) * 0.1
    bd, wd, xd = bias.cuda(), w.cuda(), buf.cuda()
    out = torch.full((m, n), float("nan"), device="cuda")
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo = xd.data_ptr(), ldx, m, n, k, L.VV_BF16, out.data_ptr(), n
    a.w, a.bias = wd.data_ptr(), bd.data_ptr()
    L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    want = x.bfloat16().float() @ w.float().T + bias
    e = rel_rms(out.cpu().numpy(), want.numpy())
    assert e < 1e-5, f"m={m} n={n} k={k} ldx={ldx}: rel RMS {e:.3e}"


@pytest.mark.parametrize("C_,T", [(512, 40), (256, 200), (512, 37), (256, 5), (512, 64), (256, 256), (512, 3), (1024, 8), (1024, 13), (1024, 4), (128, 800), (128, 45), (128, 7)])
def test_block_mid_two_launches_vs_torch(lib, C_, T):
    """vv_block_mid (middle-stage Block1D of a streaming frame as two launches: mixer + first FFN GEMM, second FFN GEMM; vv_convffn.hip)
    against the torch fp32 restatement of Block1D.forward (modular_vibevoice_tokenizer.py:555-600) on the same bf16-rounded weights:
    three consecutive streaming calls (history carried in b.hist, also when T < 6 keeps old history rows) and a stateless call, in place
    and out of place.  Tolerance: activations are rounded to bf16 at the two GEMM inputs."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(300 + C_ + T)
    r = lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc
    p = dict(gamma=r(C_, sc=0.5), ffn_gamma=r(C_, sc=0.5), norm_w=1 + r(C_, sc=0.1), ffn_norm_w=1 + r(C_, sc=0.1), dw_w=r(C_, 7, sc=0.3), dw_b=r(C_, sc=0.1),
             w1=(r(4 * C_, C_) / C_ ** 0.5).bfloat16(), b1=r(4 * C_, sc=0.1), w2=(r(C_, 4 * C_) / (4 * C_) ** 0.5).bfloat16(), b2=r(C_, sc=0.1))
    eps = 1e-5

    def rms(x, w): return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w

    def ref(x, hist):
        xn = rms(x, p["norm_w"])
        seq = torch.cat([hist, xn])
        s = p["dw_b"] + sum(p["dw_w"][:, k] * seq[k: k + x.shape[0]] for k in range(7))
        x1 = x + p["gamma"] * s
        h = torch.nn.functional.gelu(rms(x1, p["ffn_norm_w"]) @ p["w1"].float().T + p["b1"])
        return x1 + p["ffn_gamma"] * (h @ p["w2"].float().T + p["b2"]), seq[-6:]

    d = {k: v.cuda().contiguous() for k, v in p.items()}
    hist_dev = torch.zeros(6, C_, device="cuda")
    b = L.Block()
    for k in ("gamma", "ffn_gamma", "norm_w", "ffn_norm_w", "dw_w", "dw_b", "w1", "b1", "w2", "b2"):
        setattr(b, k, d[k].data_ptr())
    ws = torch.empty(l.vv_block_mid_ws_bytes(T, C_), dtype=torch.uint8, device="cuda")
    hist = torch.zeros(6, C_)
    for call in range(4):                       # calls 0-2: streaming; call 3: stateless (zero left context)
        x = r(T, C_)
        streaming = call < 3
        b.hist = hist_dev.data_ptr() if streaming else None
        want, new_hist = ref(x, hist if streaming else torch.zeros(6, C_))
        xd, od = x.cuda(), torch.full((T, C_), float("nan"), device="cuda")
        L.check(l.vv_block_mid(C.byref(b), L.VV_BF16, xd.data_ptr(), od.data_ptr(), ws.data_ptr(), T, C_, eps, None), "vv_block_mid")
        torch.cuda.synchronize()
        e = rel_rms(od.cpu().numpy(), want.numpy())
        assert e < 1e-2, f"call {call} C={C_} T={T}: rel RMS {e:.3e}"
        if streaming:
            hist = new_hist
            eh = rel_rms(hist_dev.cpu().numpy(), hist.numpy())
            assert eh < 1e-5, f"call {call} C={C_} T={T}: history rel RMS {eh:.3e}"
    # not covered -> explicit refusal, never a silent fallback
    assert l.vv_block_mid(C.byref(b), L.VV_F32, xd.data_ptr(), od.data_ptr(), ws.data_ptr(), T, C_, eps, None) != 0
    assert l.vv_block_mid(C.byref(b), L.VV_BF16, xd.data_ptr(), od.data_ptr(), ws.data_ptr(), 2, C_, eps, None) != 0


@pytest.mark.parametrize("m,n,k,dual", [(330, 2048, 1536, False), (200, 8960, 1536, True), (129, 1536, 8960, False), (128, 128, 32, False), (513, 256, 96, True),
                                        (1024, 256, 1024, False), (2500, 128, 512, False), (1300, 384, 96, True),
                                        (330, 1536, 8960, False), (203, 2048, 8192, False), (65, 3072, 2048, False), (203, 64, 14336, False), (64, 192, 8192, False)])
def test_prefill_gemm_bf16_activations(lib, m, n, k, dual):
    """vv_linear with VV_LIN_X_BF16 at prompt and voice-prompt sizes: bias / SwiGLU / residual epilogues against torch on the same bf16 operands.
    At today's thresholds (vv_linear_route) the cases reach four kernels: the 64 x 64 LDS-tiled GEMM - mfma_tiled<dual=0,bk=128,tm=64> for every
    non-dual case with K >= 1024 and n % 128 == 0 (the narrow long-K entry for n = 64 / 192), mfma_tiled<dual=1,bk=64,tm=64> for
    (200, 8960, 1536) and mfma_tiled<dual=1,bk=32,tm=64> for (1300, 384, 96) - and the direct-stream kernel with one 32-row tile per
    workgroup: mfma_stream<dual=0,ksplit=0,xb=1,mt=1> for (128, 128, 32), <dual=1,ksplit=0,xb=1,mt=1> for (513, 256, 96) and
    <dual=0,ksplit=1,xb=1,mt=1> for (1024, 256, 1024) and (2500, 128, 512).  The 128-row-strip (mt=4) kernel, the 128 x 128 tiles and every other
    instantiation are pinned, per output tile, by tests/test_hip_mfma_gemm.py; this test stays as the wide-shape net."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(m + n + k)
    x = (torch.randn(m, k, generator=g)).bfloat16()
    w = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
    w2 = (torch.randn(n, k, generator=g) / k ** 0.5).bfloat16()
    bias, res = torch.randn(n, generator=g) * 0.1, torch.randn(m, n, generator=g)
    xd, wd, w2d, bd, rd = x.cuda(), w.cuda(), w2.cuda(), bias.cuda(), res.cuda()
    out = torch.full((m, n), float("nan"), device="cuda")
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo = xd.data_ptr(), k, m, n, k, L.VV_BF16, out.data_ptr(), n
    a.w = wd.data_ptr()
    a.flags = L.LIN_X_BF16
    if dual:
        a.w2, a.act = w2d.data_ptr(), 2
        want = torch.nn.functional.silu(x.float() @ w.float().T) * (x.float() @ w2.float().T)
    else:
        a.bias, a.res, a.ldres = bd.data_ptr(), rd.data_ptr(), n
        want = x.float() @ w.float().T + bias + res
    L.check(l.vv_linear(C.byref(a), None), "vv_linear")
    torch.cuda.synchronize()
    assert rel_rms(out.cpu().numpy(), want.numpy()) < 2e-5


@pytest.mark.parametrize("m,n,k,dual", [(2, 4608, 1536, True), (2, 1536, 4608, False), (1, 2048, 8192, False), (2, 2048, 1536, False),
                                        (2, 1536, 8960, False), (2, 96, 512, False), (2, 3584, 10752, True), (1, 257, 24, False), (2, 64, 18944, False)])
def test_linear_fp8_weights(lib, m, n, k, dual):
    """Weight-only fp8 (e4m3fn codes + power-of-two row scales) on the streaming GEMV: bit pattern decode, scale, RMSNorm prologue,
    bias / SwiGLU / residual epilogues against torch on the dequantised matrix."""
    from vibevoice_rocm_amd.weights import quantize_e4m3_pow2
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(7 * m + n + k)
    x = torch.randn(m, k, generator=g)
    w, w2 = torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(n, k, generator=g) / k ** 0.5
    w[0, :8] = torch.tensor([448.0, -448.0, 2 ** -9, -2 ** -9, 0.0, 1.0, -1.75, 240.0]) * w.abs().max() / 448.0   # range ends, subnormal
    q1, s1, e1 = quantize_e4m3_pow2(w)
    q2, s2, e2 = quantize_e4m3_pow2(w2)
    assert torch.equal(e1.bfloat16().float(), e1), "dequantised weights must be exact in bf16"
    nw, bias, res = 1 + 0.1 * torch.randn(k, generator=g), 0.1 * torch.randn(n, generator=g), torch.randn(m, n, generator=g)
    d = [t.cuda() for t in (x, q1, s1, q2, s2, nw, bias, res)]
    out = torch.full((m, n), float("nan"), device="cuda")
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.n, a.k, a.wdt, a.out, a.ldo = d[0].data_ptr(), k, m, n, k, L.VV_FP8, out.data_ptr(), n
    a.w, a.wscale = d[1].data_ptr(), d[2].data_ptr()
    xn = x * torch.rsqrt((x * x).mean(-1, keepdim=True) + 1e-6) * nw
    if dual:
        a.w2, a.w2scale, a.act = d[3].data_ptr(), d[4].data_ptr(), 2
        a.pro, a.norm_w, a.eps = 1, d[5].data_ptr(), 1e-6
        want = torch.nn.functional.silu(xn @ e1.T) * (xn @ e2.T)
    else:
        a.bias, a.res, a.ldres = d[6].data_ptr(), d[7].data_ptr(), n
        want = x @ e1.T + bias + res
    L.check(l.vv_linear(C.byref(a), None), "vv_linear fp8")
    torch.cuda.synchronize()
    assert rel_rms(out.cpu().numpy(), want.numpy()) < 2e-6
    a.m = 12                                                   # GEMM-shaped: the bf16 matrix is the operand there, fp8 is refused
    assert l.vv_linear(C.byref(a), None) != 0


def test_generate_mid_fp8_weights_vs_oracle(mid):
    """weight_quant="fp8": generate() against the oracle run on the effective (dequantised) matrices - prefill (bf16 copies) and
    decode (fp8 codes) must be the same model."""
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    from vibevoice_rocm_amd.weights import fp8_effective_state_dict, fp8_matrix_names
    cfg, sd = mid
    eff = fp8_effective_state_dict(cfg, sd)
    names = set(fp8_matrix_names(cfg))
    sd_o = {k: (eff[k] if k in names else (v.to(torch.bfloat16).float() if v.dim() >= 2 else v)) for k, v in sd.items()}
    V = cfg.vocab
    ST, E, D, EOS = V - 4, V - 3, V - 2, V - 1
    special = dict(speech_start=ST, speech_end=E, speech_diffusion=D, eos=EOS)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V - 8, (70,), generator=g)            # >= 64 rows: the prompt takes the prefill (bf16 GEMM) path
    forced = [ST] + [D] * 5 + [E, EOS]
    noise = torch.randn(5, cfg.latent, generator=g)
    ref = O.generate(sd_o, cfg.as_dict(), ids.tolist(), torch.zeros(70, dtype=torch.bool), None, special, noise, cfg_scale=2.0, n_steps=10,
                     forced_tokens=forced, bf16_t=True)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="fp8")
    m.set_ddpm_inference_steps(10)
    out = m.generate(input_ids=ids[None], tokenizer=_Tok(ST, E, D, EOS), cfg_scale=2.0, forced_tokens=forced, noise=noise)
    assert out.sequences[0, 70:].tolist() == forced
    got, want = out.speech_outputs[0][0].cpu().numpy(), torch.cat(ref.audio).numpy()
    assert got.shape == want.shape == (5 * cfg.hop,)
    err = rel_rms(got, want)
    assert err < 2e-2, f"fp8 generate() vs oracle on the effective weights: rel RMS {err:.3e}"
    # and it is a different model from the unquantised one (the test would be vacuous otherwise)
    m2 = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m2.set_ddpm_inference_steps(10)
    out2 = m2.generate(input_ids=ids[None], tokenizer=_Tok(ST, E, D, EOS), cfg_scale=2.0, forced_tokens=forced, noise=noise)
    assert rel_rms(out2.speech_outputs[0][0].cpu().numpy(), got) > 5e-2


def test_linear_rejects_bad_args(lib):
    L = lib
    l = L.load()
    a = L.LinArgs()
    assert l.vv_linear(C.byref(a), None) == -1
    assert b"null" in l.vv_last_error()


# ---------------------------------------------------------------------------------------------------------------
# (1) engine components vs golden fixtures of the reference (tiny shapes)
# ---------------------------------------------------------------------------------------------------------------
def test_scheduler_tables_match_reference(tiny_engine):
    g = load_golden("scheduler")
    for n in (10, 20, 50):
        tiny_engine.set_steps(n)
        assert tiny_engine.scheduler.timesteps.tolist() == g[f"timesteps_{n}"].tolist()
        # fp32 host arithmetic (cumprod / sqrt) may differ by an ulp between the fixture box's CPU and this one
        np.testing.assert_allclose(tiny_engine.scheduler.sigmas.numpy(), g[f"sigmas_{n}"], rtol=5e-7, atol=0)


def test_head_forward_vs_reference(tiny_engine, lib):
    from vibevoice_rocm_amd.schedule import timestep_sinusoid
    L, eng = lib, tiny_engine
    g = load_golden("head_tiny")
    cfg = eng.cfg
    x, cond = dev(g["x"]), dev(g["cond"])
    ws = torch.empty(eng.lib.vv_head_ws_bytes(C.byref(eng.w.head), 8), dtype=torch.uint8, device="cuda")
    for t in (999, 500, 50):
        sin = timestep_sinusoid([t, t, t], 256).cuda()
        t1 = torch.empty(3, cfg.head_hidden, device="cuda")
        temb = torch.empty(3, cfg.head_hidden, device="cuda")
        with torch.cuda.stream(eng.stream):
            eng.linear(sin, eng.w.t_mlp0, t1)
            eng.linear(t1, eng.w.t_mlp2, temb, pro=L.PRO_SILU)
            v = torch.empty(3, cfg.latent, device="cuda")
            L.check(eng.lib.vv_head_forward(C.byref(eng.w.head), x.data_ptr(), temb.data_ptr(), cond.data_ptr(), 3, v.data_ptr(),
                                            ws.data_ptr(), eng.sp), "vv_head_forward")
        eng.stream.synchronize()
        assert rel_rms(v.cpu().numpy(), g[f"out_t{t}"]) < F32_TOL, t


def test_sample_speech_tokens_vs_reference(tiny_engine):
    eng = tiny_engine
    g = load_golden("sample_tiny")
    for n in (10, 20):
        eng.set_steps(n)
        for cs in (1.0, 1.3, 2.0):
            with torch.cuda.stream(eng.stream):
                eng.hidden2[0].copy_(dev(g["cond"][0]))
                eng.hidden2[1].copy_(dev(g["ncond"][0]))
                eng.noise_dev.copy_(dev(g["noise"][0]))
                eng._ck(eng.lib.vv_head_sample(C.byref(eng.w.head), eng.hidden2.data_ptr(), eng.cfg.hidden, eng.noise_dev.data_ptr(),
                                               eng.temb.data_ptr(), eng._coefs, n, cs, eng.latent.data_ptr(), eng._head_ws.data_ptr(), None, eng.sp),
                        "vv_head_sample")
            eng.stream.synchronize()
            assert rel_rms(eng.latent.cpu().numpy(), g[f"latent_n{n}_cfg{cs}"][0]) < 3e-4, (n, cs)


def test_sample_speech_tokens_sde_solver_vs_reference(tiny_engine):
    """The SDE solver main.py selects (scheduler.from_config(algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2"),
    main.py:543-548) against the reference's own sample_speech_tokens with the variance noise replayed."""
    from vibevoice_rocm_amd.schedule import DPMSolverMultistepScheduler
    eng = tiny_engine
    g = load_golden("sample_sde_tiny")
    ode = eng.scheduler
    eng.scheduler = DPMSolverMultistepScheduler.from_config(ode.config, algorithm_type="sde-dpmsolver++", beta_schedule="squaredcos_cap_v2")
    try:
        for n in (10, 20):
            eng.set_steps(n)
            assert eng.sde and eng._coefs[0].cn > 0 and eng._coefs[n - 1].cn == 0.0
            with torch.cuda.stream(eng.stream):
                eng.hidden2[0].copy_(dev(g["cond"][0]))
                eng.hidden2[1].copy_(dev(g["ncond"][0]))
                eng.noise_dev.copy_(dev(g["noise"][0]))
                eng.sde_noise_dev.copy_(dev(g[f"step_noise_n{n}"][:, 0]))
                eng._ck(eng.lib.vv_head_sample(C.byref(eng.w.head), eng.hidden2.data_ptr(), eng.cfg.hidden, eng.noise_dev.data_ptr(),
                                               eng.temb.data_ptr(), eng._coefs, n, 1.5, eng.latent.data_ptr(), eng._head_ws.data_ptr(),
                                               eng.sde_noise_dev.data_ptr(), eng.sp), "vv_head_sample")
            eng.stream.synchronize()
            assert rel_rms(eng.latent.cpu().numpy(), g[f"latent_n{n}"][0]) < 3e-4, n
            # a step with a noise coefficient but no noise is refused, never silently run as the ODE solver
            assert eng.lib.vv_head_sample(C.byref(eng.w.head), eng.hidden2.data_ptr(), eng.cfg.hidden, eng.noise_dev.data_ptr(), eng.temb.data_ptr(),
                                          eng._coefs, n, 1.5, eng.latent.data_ptr(), eng._head_ws.data_ptr(), None, eng.sp) != 0
    finally:
        eng.scheduler = ode
        eng.set_steps(10)


def test_generate_with_sde_solver_mid_vs_oracle(mid):
    """generate() after the main.py scheduler swap, bf16 'mid' preset, injected initial + variance noise, against the oracle."""
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg, sd = mid
    sd_o = {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 else v) for k, v in sd.items()}
    V = cfg.vocab
    ST, E, D, EOS = V - 4, V - 3, V - 2, V - 1
    g = torch.Generator().manual_seed(21)
    noise, sde_noise = torch.randn(3, cfg.latent, generator=g), torch.randn(3, 10, cfg.latent, generator=g)
    cond, ncond = torch.randn(1, cfg.hidden, generator=g), torch.randn(1, cfg.hidden, generator=g)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m.model.noise_scheduler = m.model.noise_scheduler.from_config(m.model.noise_scheduler.config, algorithm_type="sde-dpmsolver++",
                                                                  beta_schedule="squaredcos_cap_v2")
    m.set_ddpm_inference_steps(num_steps=10)
    eng = m.engine
    assert eng.sde
    W = {k[len("model.prediction_head."):]: v for k, v in sd_o.items() if k.startswith("model.prediction_head.")}
    W = {"model.prediction_head." + k: v for k, v in W.items()}
    want = O.sample_speech_tokens(sd_o, cfg.as_dict(), cond, ncond, noise[:1], 1.5, 10, algorithm="sde-dpmsolver++", sde_noise=sde_noise[0][:, None],
                                  bf16_t=True)
    with torch.cuda.stream(eng.stream):
        eng.hidden2[0].copy_(cond[0].cuda()); eng.hidden2[1].copy_(ncond[0].cuda())
    eng.cfg_scale = 1.5
    eng.step_speech(noise[0], sde_noise[0])
    eng.stream.synchronize()
    err = rel_rms(eng.latent.cpu().numpy(), want[0].numpy())
    assert err < 2e-2, f"SDE sampling bf16 vs oracle: rel RMS {err:.3e}"
    # whole loop: speculative and plain launches agree bit for bit with the SDE noise in play, and differ from the ODE solver
    ids = torch.randint(0, V - 8, (20,), generator=g)
    forced = [ST, D, D, E, ST, D, EOS]
    outs = []
    for spec in (False, True):
        m.speculative_frames = spec
        o = m.generate(input_ids=ids[None], tokenizer=_Tok(ST, E, D, EOS), cfg_scale=1.5, forced_tokens=forced, noise=noise, sde_noise=sde_noise)
        outs.append(o.speech_outputs[0][0].cpu().numpy())
    assert outs[0].shape == (3 * cfg.hop,) and np.array_equal(outs[0], outs[1])


def test_decoder_streaming_vs_reference(tiny_engine):
    eng = tiny_engine
    g = load_golden("decoder_tiny")
    with torch.cuda.stream(eng.stream):
        eng.reset_speech_caches()
    for f in range(g["latents"].shape[0]):
        with torch.cuda.stream(eng.stream):
            if f == int(g["reset_before"]):
                eng.reset_speech_caches()
            lat = dev(g["latents"][f])
            eng._ck(eng.lib.vv_decoder_forward(C.byref(eng.w.dec), lat.data_ptr(), 1, 1.0, 0.0, eng.wav.data_ptr(), eng._dec_ws.data_ptr(), eng.sp), "dec")
        eng.stream.synchronize()
        assert rel_rms(eng.wav.cpu().numpy(), g["wav_stream"][f]) < F32_TOL, f


def test_semantic_streaming_and_ragged_acoustic_vs_reference(tiny_engine):
    eng = tiny_engine
    g = load_golden("semantic_tiny")
    with torch.cuda.stream(eng.stream):
        eng.reset_speech_caches()
    for f in range(g["wav"].shape[0]):
        with torch.cuda.stream(eng.stream):
            if f == int(g["reset_before"]):
                eng.reset_speech_caches()
            wav = dev(g["wav"][f])
            eng._ck(eng.lib.vv_encoder_forward(C.byref(eng.w.sem), wav.data_ptr(), eng.cfg.hop, eng.sem.data_ptr(), eng._sem_ws.data_ptr(), eng.sp), "sem")
        eng.stream.synchronize()
        assert rel_rms(eng.sem.cpu().numpy(), g["feat_stream"][f]) < F32_TOL, f
    ac = eng.acoustic_encode(dev(g["ragged_wav"]))
    eng.stream.synchronize()
    assert tuple(ac.shape) == g["ragged_acoustic_mean"].shape
    assert rel_rms(ac.cpu().numpy(), g["ragged_acoustic_mean"]) < F32_TOL


def test_connectors_vs_reference(tiny_engine):
    eng = tiny_engine
    g = load_golden("connector_tiny")
    a = eng.connector("acoustic", dev(g["a"]))
    s = eng.connector("semantic", dev(g["s"]))
    eng.stream.synchronize()
    assert rel_rms(a.cpu().numpy(), g["a_out"]) < F32_TOL
    assert rel_rms(s.cpu().numpy(), g["s_out"]) < F32_TOL


def test_llm_prefill_decode_vs_reference(tiny_engine):
    eng = tiny_engine
    g = load_golden("llm_tiny")
    eng.begin_sequence(64, [150, 151, 152, 153])
    x0 = eng.embed_ids(torch.from_numpy(g["ids"]))
    eng.prefill(x0, row=0)
    eng.stream.synchronize()
    assert rel_rms(eng.hidden2[0].cpu().numpy(), g["prefill_hidden"][-1]) < F32_TOL
    for i in range(3):
        with torch.cuda.stream(eng.stream):
            eng.x2[0].copy_(dev(g["decode_embeds"][i]))
            eng.x2[1].copy_(dev(g["decode_embeds"][i]))
            lens = torch.tensor([12 + i, 0], dtype=torch.int32, device="cuda")
            eng.llm_forward(eng.x2, lens, None, eng.hidden2)
        eng.stream.synchronize()
        assert rel_rms(eng.hidden2[0].cpu().numpy(), g["decode_hidden"][i]) < F32_TOL, i
    k0 = eng._kv_t[0][0, 0, :, :15].cpu().numpy()
    v1 = eng._kv_t[1][1, 0, :, :15].cpu().numpy()
    assert rel_rms(k0, g["k_cache_l0"]) < F32_TOL
    assert rel_rms(v1, g["v_cache_l1"]) < F32_TOL


def _tiny_model(tiny_cfg, tiny_weights, graphs):
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    return VibeVoiceForConditionalGenerationInference(tiny_cfg, tiny_weights, device="cuda:0", torch_dtype=torch.float32, use_graphs=graphs)


class _Tok:
    def __init__(self, st, se, sd, eos):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = st, se, sd, eos
        self.bos_token_id = None
        self.pad_id = 0


@pytest.mark.parametrize("graphs", [False, True])
def test_generate_loop_vs_reference_trace(tiny_cfg, tiny_weights, graphs):
    """End-to-end drop-in check: generate() on the HIP engine against the hand-driven trace of the reference
    (voice-prompt prefill with injected noise, forced token schedule with two speech segments, CFG 1.3, 10 steps)."""
    _need_gpu()
    g = load_golden("loop_trace_tiny")
    ST, E, D, EOS = [int(v) for v in g["special"]]
    m = _tiny_model(tiny_cfg, tiny_weights, graphs)
    m.set_ddpm_inference_steps(int(g["n_steps"]))
    out = m.generate(input_ids=torch.from_numpy(g["ids"])[None], speech_tensors=torch.from_numpy(g["voice"]),
                     speech_masks=torch.from_numpy(g["speech_masks"]), speech_input_mask=torch.from_numpy(g["speech_input_mask"])[None],
                     tokenizer=_Tok(ST, E, D, EOS), cfg_scale=float(g["cfg_scale"]), forced_tokens=g["forced"].tolist(),
                     noise=torch.from_numpy(g["noise"]), speech_noise=(torch.from_numpy(g["std_noise"]), torch.from_numpy(g["eps_noise"])),
                     generation_config={"do_sample": False}, show_progress_bar=False)
    assert out.sequences[0, len(g["ids"]):].tolist() == g["tokens"].tolist()
    wav = out.speech_outputs[0]
    assert tuple(wav.shape) == (1, 5 * tiny_cfg.hop)
    ref = g["wav"].reshape(-1)
    assert rel_rms(wav[0].cpu().numpy(), ref) < 1e-3          # north_star: waveform within 1e-3 RMS (fp32)
    assert float(np.sqrt(np.mean((wav[0].cpu().numpy() - ref) ** 2))) < 1e-3


# ---------------------------------------------------------------------------------------------------------------
# (2) mid shapes vs the CPU oracle
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("mid")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 4321).items()}
    return cfg, sd


def test_speculative_frame_launch_is_exact(mid):
    """generate() with the diffusion tail launched speculatively behind every LLM step (and rolled back when the token is not
    speech_diffusion: speech_end, a speech_start straight after a frame, EOS) must reproduce the non-speculative run bit for bit."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg, sd = mid
    V = cfg.vocab
    ST, E, D, EOS = V - 4, V - 3, V - 2, V - 1
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V - 8, (24,), generator=g)
    forced = [ST, D, D, ST, D, D, D, E, ST, D, E, ST, D, D, EOS]
    noise = torch.randn(16, cfg.latent, generator=g)
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16)
    m.set_ddpm_inference_steps(10)
    outs = []
    for spec in (False, True, True):
        m.speculative_frames = spec
        out = m.generate(input_ids=ids[None], tokenizer=_Tok(ST, E, D, EOS), cfg_scale=1.5, forced_tokens=forced, noise=noise)
        outs.append((out.sequences[0].tolist(), out.speech_outputs[0][0].cpu().numpy()))
    assert outs[0][0] == outs[1][0] == outs[2][0]
    assert outs[0][1].shape == (8 * cfg.hop,)
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[1][1], outs[2][1])


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-3), (torch.bfloat16, 2e-2)])
def test_generate_mid_vs_oracle(mid, dtype, tol):
    from oracle import vv_oracle as O
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference
    cfg, sd = mid
    if dtype == torch.bfloat16:     # oracle on the same bf16-rounded matrices, fp32 arithmetic
        sd_o = {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 else v) for k, v in sd.items()}
    else:
        sd_o = sd
    V = cfg.vocab
    ST, E, D, EOS = V - 4, V - 3, V - 2, V - 1
    special = dict(speech_start=ST, speech_end=E, speech_diffusion=D, eos=EOS)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, V - 8, (40,), generator=g)
    forced = [ST] + [D] * 6 + [E, ST] + [D] * 3 + [E, EOS]
    noise = torch.randn(9, cfg.latent, generator=g)
    voice = 0.1 * torch.randn(1, 2 * cfg.hop + 999, generator=g)
    sp_mask = torch.zeros(40, dtype=torch.bool)
    sp_mask[5:8] = True
    speech_masks = torch.ones(1, 3, dtype=torch.bool)
    std_noise, eps_noise = torch.randn(1, generator=g), torch.randn(1, 3, cfg.ac_dim, generator=g)
    ocfg = cfg.as_dict()
    _, conn = O.process_speech_inputs(sd_o, ocfg, voice, speech_masks, std_noise, eps_noise)
    ref = O.generate(sd_o, ocfg, ids.tolist(), sp_mask, conn, special, noise, cfg_scale=2.0, n_steps=20, forced_tokens=forced,
                     bf16_t=(dtype == torch.bfloat16))      # the bf16 engine keeps its default: t and the sinusoid rounded like the reference's bf16 run
    m = VibeVoiceForConditionalGenerationInference(cfg, sd, device="cuda:0", torch_dtype=dtype)
    assert m.engine.bf16_t_quirk == (dtype == torch.bfloat16)
    m.set_ddpm_inference_steps(20)
    out = m.generate(input_ids=ids[None], speech_tensors=voice, speech_masks=speech_masks, speech_input_mask=sp_mask[None],
                     tokenizer=_Tok(ST, E, D, EOS), cfg_scale=2.0, forced_tokens=forced, noise=noise, speech_noise=(std_noise, eps_noise))
    assert out.sequences[0, 40:].tolist() == forced
    ref_wav = torch.cat(ref.audio).numpy()
    got = out.speech_outputs[0][0].cpu().numpy()
    assert got.shape == ref_wav.shape == (9 * cfg.hop,)
    err = rel_rms(got, ref_wav)
    assert err < tol, f"generate() {dtype} vs oracle: waveform rel RMS {err:.3e} (bar {tol})"


@pytest.mark.parametrize("heads,kv_heads,d,kvdt,R,pos0", [(12, 2, 128, "bf16", 77, 0), (12, 2, 128, "f32", 21, 5), (28, 4, 128, "bf16", 40, 3),
                                                        (4, 2, 16, "f32", 19, 0), (4, 2, 128, "bf16", 9, 130), (6, 2, 128, "bf16", 33, 0)])
def test_prompt_attention_vs_torch(lib, heads, kv_heads, d, kvdt, R, pos0):
    """vv_attn at prompt row counts (causal: row r sees keys 0..pos0+r of one cache row).  GQA ratios 6 / 7 / 2 take the kernel that
    shares K/V loads across the q heads of a group, ratio 3 the per-head kernel; both against a softmax in torch fp32 on the same
    cache contents (reference call site: Qwen2 attention under modeling_vibevoice_inference.py:226-237)."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(heads * 100 + R)
    layers, rows, s_max, layer = 2, 2, pos0 + R + 3, 1
    tdt = torch.bfloat16 if kvdt == "bf16" else torch.float32
    kc = torch.randn(layers, rows, kv_heads, s_max, d, generator=g).to(tdt)
    vc = torch.randn(layers, rows, kv_heads, s_max, d, generator=g).to(tdt)
    ld = (heads + 2 * kv_heads) * d
    qkv = torch.randn(R, ld, generator=g)
    lens = torch.arange(pos0, pos0 + R, dtype=torch.int32)
    crow = torch.ones(R, dtype=torch.int32)
    kd, vd, qd, ld_, cd = kc.cuda(), vc.cuda(), qkv.cuda(), lens.cuda(), crow.cuda()
    out = torch.full((R, heads * d), float("nan"), device="cuda")
    kv = L.KV(kd.data_ptr(), vd.data_ptr(), L.VV_BF16 if kvdt == "bf16" else L.VV_F32, layers, rows, kv_heads, s_max, d)
    L.check(l.vv_attn(qd.data_ptr(), ld, R, heads, C.byref(kv), layer, ld_.data_ptr(), cd.data_ptr(), out.data_ptr(), heads * d, None), "vv_attn")
    torch.cuda.synchronize()
    q = qkv[:, :heads * d].view(R, heads, d)
    want = torch.empty(R, heads, d)
    for h in range(heads):
        kh = kc[layer, 1, h // (heads // kv_heads)].float()
        vh = vc[layer, 1, h // (heads // kv_heads)].float()
        sc = (q[:, h] @ kh.T) / d ** 0.5
        mask = torch.arange(s_max)[None, :] > lens[:, None]
        sc = sc.masked_fill(mask, float("-inf"))
        want[:, h] = torch.softmax(sc, -1) @ vh
    assert rel_rms(out.cpu().numpy(), want.reshape(R, -1).numpy()) < 2e-6


@pytest.mark.parametrize("heads,kv_heads,R,pos0", [(12, 2, 77, 0), (28, 4, 40, 3), (12, 2, 330, 0), (12, 2, 64, 500), (4, 2, 33, 130), (12, 2, 16, 0)])
def test_prompt_attention_matrix_core_vs_torch(lib, heads, kv_heads, R, pos0):
    """vv_attn with a transposed value cache (vv_kv.vt): QK^T and PV on mfma_f32_32x32x16_bf16, one wave per (32-query tile, q head), causal
    (row r sees keys 0..pos0+r), ragged last tile, a second chunk on top of 500 cached keys, GQA 6 / 7 / 2.  Q and P are rounded to bf16 for
    the matrix cores (as FlashAttention-2 in the reference's bf16 run does): 5e-3 against a torch fp32 softmax on the same cache contents."""
    L = lib
    l = L.load()
    g = torch.Generator().manual_seed(heads * 100 + R + pos0)
    d, layers, rows, layer = 128, 2, 2, 1
    s_max = (pos0 + R + 3 + 31) // 32 * 32
    kc = torch.randn(layers, rows, kv_heads, s_max, d, generator=g).to(torch.bfloat16)
    vc = torch.randn(layers, rows, kv_heads, s_max, d, generator=g).to(torch.bfloat16)
    ld = (heads + 2 * kv_heads) * d
    qkv = torch.randn(R, ld, generator=g)
    lens = torch.arange(pos0, pos0 + R, dtype=torch.int32)
    crow = torch.ones(R, dtype=torch.int32)
    kd, vd, vtd, qd, ld_, cd = kc.cuda(), vc.cuda(), vt_tiles(vc).cuda(), qkv.cuda(), lens.cuda(), crow.cuda()
    out = torch.full((R, heads * d), float("nan"), device="cuda")
    kv = L.KV(kd.data_ptr(), vd.data_ptr(), L.VV_BF16, layers, rows, kv_heads, s_max, d, vtd.data_ptr())
    L.check(l.vv_attn(qd.data_ptr(), ld, R, heads, C.byref(kv), layer, ld_.data_ptr(), cd.data_ptr(), out.data_ptr(), heads * d, None), "vv_attn")
    torch.cuda.synchronize()
    q = qkv[:, :heads * d].view(R, heads, d)
    want = torch.empty(R, heads, d)
    for h in range(heads):
        kh = kc[layer, 1, h // (heads // kv_heads)].float()
        vh = vc[layer, 1, h // (heads // kv_heads)].float()
        sc = (q[:, h] @ kh.T) / d ** 0.5
        sc = sc.masked_fill(torch.arange(s_max)[None, :] > lens[:, None], float("-inf"))
        want[:, h] = torch.softmax(sc, -1) @ vh
    err = rel_rms(out.cpu().numpy(), want.reshape(R, -1).numpy())
    assert err < 5e-3, f"matrix-core prompt attention vs torch: rel RMS {err:.3e}"
    # the VALU kernels on the same inputs (vt = NULL) agree with the matrix-core path to bf16 rounding of Q / P
    kv2 = L.KV(kd.data_ptr(), vd.data_ptr(), L.VV_BF16, layers, rows, kv_heads, s_max, d)
    out2 = torch.empty_like(out)
    L.check(l.vv_attn(qd.data_ptr(), ld, R, heads, C.byref(kv2), layer, ld_.data_ptr(), cd.data_ptr(), out2.data_ptr(), heads * d, None), "vv_attn")
    torch.cuda.synchronize()
    assert rel_rms(out.cpu().numpy(), out2.cpu().numpy()) < 5e-3
