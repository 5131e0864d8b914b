"""The speech connectors against plain fp64, through the C ABI only, with vv_connector structs filled by hand - no engine, no model weights.

  vv_connector_pair        conn_fc1_pair_kernel + conn_fc2_pair_kernel<KU> at H = 512 KU for every KU = 1..7 the library compiles (din 64 / 128),
                           and one case at din_a + din_s = 512, the staging array's size; rows_out 1 / 2 / 3 into ldo > H with NaN gaps and
                           guard rows; the workspace is exactly 2 H floats between guards; two runs are bit-identical
                           the fall-backs - fp32 weights, H % 512 != 0, KU = 8, a missing bias, a 4-byte-misaligned norm_w - take the two-call
                           path (vv_prof_end then shows vv_linear launches, the fused path shows none) and are held to the same reference
  vv_connector_forward     R = 1, 2, 9, 70 with and without `accumulate`
  vv_connector_pair_rows   B = 2, 5, 8 with a mixed `active` mask: inactive dialogues' rows keep the sentinel

Reference: `conn_ref`, fp64 on the weights as the device holds them (bf16 widened exactly).  Stand-in (CPU): the same function in fp32, with the
activations of a linear rounded to bf16 once where vv_linear_route names a matrix-core kernel for it (mfma_* and skinny round x to bf16 once,
tests/test_hip_mfma_gemm.py, tests/test_hip_gemm_f32.py); every other route keeps fp32 activations.

Figures per call: rel RMS of every output row against its reference row (worst row), and the worst element, |got - ref| / rms(ref row).
Bars, one per class, by the house rule of test_hip_conv_stream.py::test_bars_sit_between_floor_and_faults (held by test_bars_sit_between_floor_and_faults
here): >= 8 x the stand-in's error against fp64, <= 1/10 of what each fault costs the worst row -
  unit    one 512-column unit of fc2's K dropped           (every class)
  swap    the two norm weights exchanged                   (pair and pair_rows: one connector has no second norm)
  ragged  a row of the last rows_per_wave round not stored (pair: the element keeps the NaN it held - any bar sees it)
The element figure's bar is ELEM x the row bar: the errors of a row's H <= 4096 elements are near-normal, their largest is about 3.7 sigma.

Measured on the MI355X (profiles/connector_parity.txt), largest value over the class's calls:
  class      comparisons                               bar row / element    largest row / element    bar / largest
  f32 act    34 (pair 24 + 5 fall-backs, forward 4,    2e-5 / 1e-4          3.19e-7 / 1.23e-6        63 / 81
             pair_rows B = 2)
  bf16 act   6 (forward R = 9, 70; pair_rows B = 5, 8) 2.5e-2 / 1.25e-1     2.58e-3 / 1.02e-2        10 / 12
Within a factor of ten of its bar: the bf16 class's row figure, 2.58e-3 against 2.5e-2 = 9.7 x (forward R = 9, 70).  Its level is the bf16 rounding of the activations itself (the CPU
stand-in gives the same 2.6e-3), and the bar's window between 8 x that floor and a tenth of the cheapest fault is narrow.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest
import torch

from conftest import rel_rms

gpu = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
VV_F32, VV_BF16 = 0, 1
EPS = 1e-6
SENT32 = 0x7FC0BEEF          # NaN bit pattern: gaps, guard rows, workspace guards, unwritten outputs

FLOOR_HEADROOM, FAULT_MARGIN = 8, 10
BAR = {"f32": 2e-5,           # fp32 products and sums over K <= 4096 on exact operands
       "bf16": 2.5e-2}        # activations rounded to bf16 once per linear: the stand-in's worst row is 2.6e-3 (fc1 sums K = 64 .. 128 terms only, so
                              # its rounding noise averages little before the norm), the cheapest fault costs 4.2e-1
ELEM = 5                      # element bar = ELEM x row bar


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_LIB = []


def _lib():
    if not _LIB:
        from vibevoice_rocm_amd import _lib as L
        l = L.load()
        if torch.cuda.is_available():
            L.check(l.vv_init(), "vv_init")
        _LIB.extend((L, l))
    return _LIB


# ---------------------------------------------------------------------------------------------------------------
# weights (CPU), the reference and the stand-in
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conn_weights(name, H, din, wdt=VV_BF16, bias=True):
    """one connector's parameters as the device will hold them (fp32 tensors; matrices bf16-exact when wdt is bf16).  The norm weight is spread
    wide (1 + 0.5 z) so that two connectors' norms are told apart"""
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{H}/{din}".encode()))
    rt = (lambda t: t.to(BF16).float()) if wdt == VV_BF16 else (lambda t: t)
    w = dict(fc1=rt(torch.randn(H, din, generator=g) * 0.8 / din ** 0.5), b1=0.1 * torch.randn(H, generator=g),
             norm_w=1.0 + 0.5 * torch.randn(H, generator=g), fc2=rt(torch.randn(H, H, generator=g) * 0.8 / H ** 0.5),
             b2=0.1 * torch.randn(H, generator=g), H=H, din=din, wdt=wdt)
    if not bias:
        w["b1"] = None
    return w


def conn_ref(w, x, dtype=torch.float64, rnd1=None, rnd2=None, fault=None, norm_w=None):
    """SpeechConnector: fc2(RMSNorm(fc1 x + b1) * norm_w) + b2 for rows x[R, din].  dtype / rnd1 / rnd2 turn it into the stand-in: rnd1 rounds
    fc1's activations, rnd2 fc2's.  fault ("unit", u): fc2's columns [512 u, 512 u + 512) contribute nothing"""
    x = x.to(dtype)
    if rnd1:
        x = rnd1(x)
    t = x @ w["fc1"].to(dtype).T
    if w["b1"] is not None:
        t = t + w["b1"].to(dtype)
    y = t * torch.rsqrt((t * t).mean(-1, keepdim=True) + EPS) * (w["norm_w"] if norm_w is None else norm_w).to(dtype)
    if rnd2:
        y = rnd2(y)
    if fault and fault[0] == "unit":
        y = y.clone()
        y[:, 512 * fault[1]: 512 * fault[1] + 512] = 0
    return (y @ w["fc2"].to(dtype).T + w["b2"].to(dtype)).double()


def pair_ref(wa, ws, xa, xs, **kw):
    fault = kw.pop("fault", None)
    na, ns = (ws["norm_w"], wa["norm_w"]) if fault == ("swap",) else (None, None)
    f = fault if fault and fault[0] == "unit" else None
    return conn_ref(wa, xa, norm_w=na, fault=f, **kw) + conn_ref(ws, xs, norm_w=ns, **kw)


def rnd_bf16(t):
    return t.to(BF16).to(t.dtype)


def _inputs(name, R, din):
    g = torch.Generator().manual_seed(zlib.crc32(f"x/{name}/{R}/{din}".encode()))
    return torch.randn(R, din, generator=g)


def row_figures(got, ref):
    """(worst row rel RMS, worst element as |err| / rms(ref row)) of got[R, H] against ref[R, H]; NaN in got gives inf"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.where(np.isfinite(got), got - ref, np.inf)
    rms = np.sqrt((ref ** 2).mean(-1))
    with np.errstate(over="ignore", invalid="ignore"):
        return float((np.sqrt((err ** 2).mean(-1)) / rms).max()), float((np.abs(err).max(-1) / rms).max())


def route_rounds(m, n, k, wdt, pro, res, ldx=None):
    """does the kernel vv_linear takes for this call round its activations to bf16 (the matrix-core GEMMs and the skinny GEMM)?  Host only."""
    L, l = _lib()
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.pro, a.eps = 0x10000, ldx or k, m, (L.PRO_RMSNORM if pro else L.PRO_NONE), EPS
    a.norm_w = 0x20000 if pro else None
    a.w, a.bias, a.n, a.k, a.wdt, a.out, a.ldo = 0x30000, 0x40000, n, k, wdt, 0x50000, n
    if res:
        a.res, a.ldres = 0x50000, n
    buf = C.create_string_buffer(128)
    L.check(l.vv_linear_route(C.byref(a), buf, 128), "vv_linear_route")
    name = buf.value.decode()
    assert name.startswith(("gemv_", "gemm_f32", "mfma_", "skinny")), name
    return name.startswith(("mfma_", "skinny"))


def klass_of(w, R, accumulate=False, ldx=None):
    """(class, rnd1, rnd2) of a connector's two linears at R rows (ldx: the pitch of fc1's input rows when it is not din)"""
    r1 = route_rounds(R, w["H"], w["din"], w["wdt"], False, False, ldx)
    r2 = route_rounds(R, w["H"], w["H"], w["wdt"], True, accumulate)
    return ("bf16" if r1 or r2 else "f32"), (rnd_bf16 if r1 else None), (rnd_bf16 if r2 else None)


# the shapes of the GPU tests, shared with the bar test
PAIR_SHAPES = [(512 * ku, 64, 128) for ku in range(1, 8)] + [(1024, 384, 128)]
FORWARD_ROWS = (1, 2, 9, 70)
ROWS_B = (2, 5, 8)
H_FWD, H_ROWS = 1024, 1536
LD_LAT, LD_FEAT = 64 + 4, 128 + 8      # pair_rows: the pitches of the latent and feature rows


def test_routes_of_the_shapes_used():
    """the classes the bars are set for: every pair / <= 8-row call keeps fp32 activations, 9 and 70 rows on bf16 weights round them"""
    w = conn_weights("fwd", H_FWD, 128)
    assert [klass_of(w, R)[0] for R in FORWARD_ROWS] == ["f32", "f32", "bf16", "bf16"]
    assert klass_of(conn_weights("fwd32", H_FWD, 128, VV_F32), 70)[0] == "f32"
    for H, da, ds in PAIR_SHAPES:
        assert klass_of(conn_weights("a", H, da), 1)[0] == "f32" and klass_of(conn_weights("s", H, ds), 1)[0] == "f32"


def test_reference_agrees_with_the_oracle():
    """conn_ref in fp32 against oracle.vv_oracle's connector on the golden-free synthetic weights: the reference restates the same module"""
    from oracle import vv_oracle as O
    w = conn_weights("orc", 512, 64, VV_F32)
    sd = {"c.fc1.weight": w["fc1"], "c.fc1.bias": w["b1"], "c.norm.weight": w["norm_w"], "c.fc2.weight": w["fc2"], "c.fc2.bias": w["b2"]}
    x = _inputs("orc", 3, 64)
    want = O.connector(sd, "c.", x)
    e = rel_rms(conn_ref(w, x).numpy(), want.double().numpy(), "conn_ref fp64 vs the fp32 oracle connector (CPU)")
    assert e < 1e-6, e


@pytest.mark.parametrize("klass", ["f32", "bf16"])
def test_bars_sit_between_floor_and_faults(klass):
    """condition 1: BAR[class] >= 8 x the stand-in's worst row against fp64 (and ELEM x BAR >= 8 x its worst element); condition 2: BAR[class] <=
    1/10 of each fault's cost to the worst row.  `ragged` leaves NaN in an element: its cost is infinite under either figure."""
    floors, costs = [], {}
    if klass == "f32":
        for H, da, ds in PAIR_SHAPES:
            wa, ws, xa, xs = conn_weights("a", H, da), conn_weights("s", H, ds), _inputs("a", 1, da), _inputs("s", 1, ds)
            want = pair_ref(wa, ws, xa, xs)
            floors.append(row_figures(pair_ref(wa, ws, xa, xs, dtype=F32), want))
            costs[f"swap H={H}"] = row_figures(pair_ref(wa, ws, xa, xs, dtype=F32, fault=("swap",)), want)[0]
            for u in (0, H // 512 - 1):
                costs[f"unit {u} H={H}"] = row_figures(pair_ref(wa, ws, xa, xs, dtype=F32, fault=("unit", u)), want)[0]
            bad = pair_ref(wa, ws, xa, xs, dtype=F32).clone()
            bad[0, H - 1] = float("nan")
            costs[f"ragged H={H}"] = row_figures(bad, want)[1]
        w = conn_weights("fwd", H_FWD, 128)
        for R in (1, 2):
            x = _inputs("fwd", R, 128)
            floors.append(row_figures(conn_ref(w, x, dtype=F32), conn_ref(w, x)))
    else:
        w = conn_weights("fwd", H_FWD, 128)
        for R in (9, 70):
            k, r1, r2 = klass_of(w, R)
            assert k == "bf16"
            x = _inputs("fwd", R, 128)
            want = conn_ref(w, x)
            floors.append(row_figures(conn_ref(w, x, dtype=F32, rnd1=r1, rnd2=r2), want))
            for u in (0, 1):
                costs[f"unit {u} R={R}"] = row_figures(conn_ref(w, x, dtype=F32, rnd1=r1, rnd2=r2, fault=("unit", u)), want)[0]
        for B in ROWS_B:
            wa, ws = conn_weights("a", H_ROWS, 64), conn_weights("s", H_ROWS, 128)
            (ka, a1, a2), (ks, s1, s2) = klass_of(wa, B, ldx=LD_LAT), klass_of(ws, B, True, ldx=LD_FEAT)
            if "bf16" not in (ka, ks):
                continue
            xa, xs = _inputs("a", B, 64), _inputs("s", B, 128)
            want = pair_ref(wa, ws, xa, xs)
            run = lambda **kw: conn_ref(wa, xa, dtype=F32, rnd1=a1, rnd2=a2, **kw.get("a", {})) + conn_ref(ws, xs, dtype=F32, rnd1=s1, rnd2=s2, **kw.get("s", {}))
            floors.append(row_figures(run(), want))
            costs[f"swap B={B}"] = row_figures(run(a=dict(norm_w=ws["norm_w"]), s=dict(norm_w=wa["norm_w"])), want)[0]
            costs[f"unit B={B}"] = row_figures(run(s=dict(fault=("unit", 2))), want)[0]
    f_row, f_el = max(f[0] for f in floors), max(f[1] for f in floors)
    print(f"{klass}: stand-in floor row {f_row:.2e} element {f_el:.2e}; bar {BAR[klass]:.1e} / {ELEM * BAR[klass]:.1e}")
    assert BAR[klass] >= FLOOR_HEADROOM * f_row and ELEM * BAR[klass] >= FLOOR_HEADROOM * f_el, (f_row, f_el)
    assert costs
    for name, c in costs.items():
        print(f"{klass}: fault {name:<16} costs {c:.2e}")
        assert BAR[klass] <= c / FAULT_MARGIN, (name, c)


# ---------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32)


def _sent(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(F32)


class DevConn:
    """a vv_connector on the device, its tensors kept alive; snapshot() / unchanged() hold the parameters bit for bit"""

    def __init__(self, w, misalign_norm=False):
        L, _ = _lib()
        wd = BF16 if w["wdt"] == VV_BF16 else F32
        self.t = dict(fc1=w["fc1"].to(wd).cuda(), fc2=w["fc2"].to(wd).cuda(), b2=w["b2"].cuda())
        if w["b1"] is not None:
            self.t["b1"] = w["b1"].cuda()
        if misalign_norm:
            buf = torch.zeros(w["H"] + 1, device="cuda")
            buf[1:] = w["norm_w"].cuda()
            self.t["norm_w"] = buf[1:]
            assert self.t["norm_w"].data_ptr() % 16 == 4
        else:
            self.t["norm_w"] = w["norm_w"].cuda()
        c = L.Connector()
        c.wdt, c.din, c.hidden = w["wdt"], w["din"], w["H"]
        c.fc1, c.b1, c.norm_w, c.fc2, c.b2 = (L.ptr(self.t.get(k)) or None for k in ("fc1", "b1", "norm_w", "fc2", "b2"))
        self.c = c
        self.snap = {k: v.clone() for k, v in self.t.items()}

    def unchanged(self):
        return all(torch.equal(v.view(torch.uint8), self.snap[k].view(torch.uint8)) for k, v in self.t.items())


class Guarded:
    """n floats between two guard regions of `guard` floats, everything NaN (SENT32) before the call"""

    def __init__(self, n, guard):
        self.n, self.g = n, guard
        self.buf = _sent(n + 2 * guard)
        self.ptr = self.buf.data_ptr() + 4 * guard

    def body(self):
        return self.buf[self.g: self.g + self.n]

    def guards_intact(self):
        b = _bits(self.buf)
        return bool((b[: self.g] == SENT32).all()) and bool((b[self.g + self.n:] == SENT32).all())


def _linear_launches(fn):
    """run fn under the vv_linear profiler: the number of vv_linear launches it made"""
    L, l = _lib()
    L.check(l.vv_prof_begin(64), "vv_prof_begin")
    try:
        fn()
    finally:
        ents = (L.ProfEntry * 64)()
        cnt = C.c_int(0)
        L.check(l.vv_prof_end(ents, 64, C.byref(cnt)), "vv_prof_end")
    return sum(ents[i].count for i in range(cnt.value))


def _hold(tag, klass, got, want):
    row, el = row_figures(got, want)
    rel_rms(np.asarray(got, dtype=np.float64), want.numpy(), tag)
    print(f"PARITY connector {klass:<5} {tag:<64} row {row:.3e} element {el:.3e}  bars {BAR[klass]:.1e} / {ELEM * BAR[klass]:.1e}")
    assert row < BAR[klass], f"{tag}: worst row {row:.3e} >= {BAR[klass]:.1e}"
    assert el < ELEM * BAR[klass], f"{tag}: worst element {el:.3e} >= {ELEM * BAR[klass]:.1e}"


def _run_pair(wa, ws, rows_out, tag, fused, misalign=False):
    L, l = _lib()
    H = wa["H"]
    da, ds = DevConn(wa, misalign_norm=misalign), DevConn(ws)
    xa, xs = _inputs("a", 1, wa["din"]), _inputs("s", 1, ws["din"])
    dxa, dxs = xa.cuda(), xs.cuda()
    want = pair_ref(wa, ws, xa, xs)
    ldo = H + 8
    outs = []
    for run in range(2):
        out = _sent(rows_out + 2, ldo)                # one guard row in front, one behind
        ws_buf = Guarded(2 * H, 2 * H)
        call = lambda: L.check(l.vv_connector_pair(C.byref(da.c), C.byref(ds.c), dxa.data_ptr(), dxs.data_ptr(), out[1].data_ptr(), ldo, rows_out,
                                                   ws_buf.ptr, None), "vv_connector_pair")
        n_lin = _linear_launches(call) if run == 0 else call()
        torch.cuda.synchronize()
        if run == 0:
            assert (n_lin == 0) == fused, f"{tag}: {n_lin} vv_linear launches: the call took the {'two-call' if n_lin else 'fused'} path"
        assert ws_buf.guards_intact(), f"{tag}: a workspace guard was written (the workspace is 2 H floats)"
        o = out.cpu()
        ob = _bits(o)
        assert bool((ob[0] == SENT32).all()) and bool((ob[-1] == SENT32).all()), f"{tag}: a guard row was written"
        assert bool((ob[1:-1, H:] == SENT32).all()), f"{tag}: the pitch gap was written"
        for r in range(1, rows_out):
            assert torch.equal(ob[1 + r, :H], ob[1, :H]), f"{tag}: output row {r} differs from row 0"
        outs.append(o[1:-1, :H])
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{tag}: two runs differ"
    assert da.unchanged() and ds.unchanged() and torch.equal(dxa.cpu(), xa) and torch.equal(dxs.cpu(), xs), f"{tag}: an input or a parameter changed"
    _hold(tag, "f32", outs[0][:1], want)


PAIR_CASES = [(H, da, ds, ro) for (H, da, ds) in PAIR_SHAPES for ro in (1, 2, 3)]


@gpu
@pytest.mark.parametrize("H,din_a,din_s,rows_out", PAIR_CASES, ids=[f"H{h}_din{a}+{s}_rows{r}" for h, a, s, r in PAIR_CASES])
def test_pair_fused_vs_fp64(H, din_a, din_s, rows_out):
    _need_gpu()
    _run_pair(conn_weights("a", H, din_a), conn_weights("s", H, din_s), rows_out, f"pair H={H} din={din_a}+{din_s} rows_out={rows_out}", fused=True)


FALLBACKS = {"fp32_weights": dict(H=1024, wdt=VV_F32), "H_520": dict(H=520), "KU_8": dict(H=4096), "no_bias": dict(H=1024, bias=False),
             "misaligned_norm_w": dict(H=1024, misalign=True)}


@gpu
@pytest.mark.parametrize("name", list(FALLBACKS))
def test_pair_fallbacks_vs_fp64(name):
    _need_gpu()
    o = dict(FALLBACKS[name])
    H, wdt, bias, mis = o["H"], o.get("wdt", VV_BF16), o.get("bias", True), o.get("misalign", False)
    wa, ws = conn_weights("a", H, 64, wdt, bias), conn_weights("s", H, 128, wdt)
    assert klass_of(wa, 1)[0] == "f32" and klass_of(ws, 1, True)[0] == "f32"
    _run_pair(wa, ws, 2, f"pair fall-back {name}", fused=False, misalign=mis)


@gpu
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("R", FORWARD_ROWS)
def test_forward_vs_fp64(R, accumulate):
    _need_gpu()
    L, l = _lib()
    w = conn_weights("fwd", H_FWD, 128)
    klass = klass_of(w, R, bool(accumulate))[0]
    d = DevConn(w)
    x = _inputs("fwd", R, 128)
    g = torch.Generator().manual_seed(R)
    base = torch.randn(R, H_FWD, generator=g)
    want = conn_ref(w, x) + (base.double() if accumulate else 0)
    dx = x.cuda()
    outs = []
    for run in range(2):
        out = _sent(R + 2, H_FWD)
        if accumulate:
            out[1:-1] = base.cuda()
        ws_buf = Guarded(R * H_FWD, R * H_FWD)
        L.check(l.vv_connector_forward(C.byref(d.c), dx.data_ptr(), R, out[1].data_ptr(), accumulate, ws_buf.ptr, None), "vv_connector_forward")
        torch.cuda.synchronize()
        assert ws_buf.guards_intact(), "a workspace guard was written (the workspace is R x hidden floats)"
        o = out.cpu()
        assert bool((_bits(o)[0] == SENT32).all()) and bool((_bits(o)[-1] == SENT32).all()), "a guard row was written"
        outs.append(o[1:-1])
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs differ"
    assert d.unchanged() and torch.equal(dx.cpu(), x)
    _hold(f"forward R={R} accumulate={accumulate}", klass, outs[0], want)


@gpu
@pytest.mark.parametrize("B", ROWS_B)
def test_pair_rows_vs_fp64(B):
    _need_gpu()
    L, l = _lib()
    H, rows_out = H_ROWS, 2
    wa, ws = conn_weights("a", H, 64), conn_weights("s", H, 128)
    klass = "bf16" if "bf16" in (klass_of(wa, B, ldx=LD_LAT)[0], klass_of(ws, B, True, ldx=LD_FEAT)[0]) else "f32"
    da, ds = DevConn(wa), DevConn(ws)
    xa, xs = _inputs("a", B, 64), _inputs("s", B, 128)
    want = pair_ref(wa, ws, xa, xs)
    active = [int(b % 3 != 1) for b in range(B)]          # dialogue 1, 4, 7 inactive
    ld_lat, ld_feat, ld_out = LD_LAT, LD_FEAT, H + 4
    lat, feat = _sent(B, ld_lat), _sent(B, ld_feat)
    lat[:, :64], feat[:, :128] = xa.cuda(), xs.cuda()
    act = torch.tensor(active, dtype=torch.int32, device="cuda")
    outs = []
    for run in range(2):
        out = _sent(B * rows_out + 2, ld_out)
        ws_buf = Guarded(2 * B * H, 2 * B * H)
        L.check(l.vv_connector_pair_rows(C.byref(da.c), C.byref(ds.c), lat.data_ptr(), ld_lat, feat.data_ptr(), ld_feat, act.data_ptr(),
                                         out[1].data_ptr(), ld_out, rows_out, B, ws_buf.ptr, None), "vv_connector_pair_rows")
        torch.cuda.synchronize()
        assert ws_buf.guards_intact(), "a workspace guard was written (the workspace is 2 B hidden floats)"
        o = out.cpu()
        ob = _bits(o)
        assert bool((ob[0] == SENT32).all()) and bool((ob[-1] == SENT32).all()) and bool((ob[:, H:] == SENT32).all()), "a guard row or the gap was written"
        outs.append(o[1:-1, :H].reshape(B, rows_out, H))
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), "two runs differ"
    assert da.unchanged() and ds.unchanged() and act.cpu().tolist() == active
    got = outs[0]
    for b in range(B):
        if active[b]:
            assert torch.equal(_bits(got[b, 1]), _bits(got[b, 0])), f"dialogue {b}: its two rows differ"
        else:
            assert bool((_bits(got[b]) == SENT32).all()), f"inactive dialogue {b}: a row was written"
    on = [b for b in range(B) if active[b]]
    _hold(f"pair_rows B={B} active={''.join(map(str, active))}", klass, got[on, 0], want[on])
