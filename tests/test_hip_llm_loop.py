"""The LLM layer loop (llm_forward in csrc/vv_model.hip, behind vv_llm_forward and vv_llm_prefill_packed) against one plain fp64 reference -
through the C ABI and the package's own builder (DeviceWeights, ensure_frag, synth_state_dict_torch); no Engine, no RowBatch.

Models.  Geometry A is the `mid` preset's LLM (hidden 512, inter 1536, 4 heads on 2 KV heads, head_dim 128) with 2 layers - layer 0 reads x where
it lies, layer 1 reads h - and the smallest vocabulary and head depth the builder is used with.  Geometry B has 12 heads on 2 KV heads: q width
1536 != hidden 512, qkv width 2048, which separates every place the loop could confuse qd, H and qkvd.  The q / k / v biases of the synthetic
state dict are scaled by 20 (std 0.4) and the norm weights' spread by 5 (std 0.5) so that a dropped bias and exchanged norm weights show.

Reference.  `run_llm(weights, x, positions, cache_rows, cache)`: a restatement of oracle/vv_oracle.py::llm_forward in fp64 with per-row positions
and cache rows; it knows nothing of regimes, tiles or workspaces.  cache_rows None is the decode convention of tests/test_hip_attn_decode.py
(ref_decode_fp64: row r owns cache row r, the new token's rotated k and v enter the step unrounded and are appended rounded to the cache type),
a list the prompt convention of tests/test_hip_attn_prefill.py (ref_rope_store_fp64 stores first, rounded; ref_prompt_fp64 reads the cache) -
both imported, not restated.  Weights go in as the device holds them.  On an fp8 cache (quantize_cache, with the code and scale rules imported
from tests/test_hip_kv_fp8.py) the cache holds code x scale and a decode step appends saturating e4m3 codes under the head's scale.
The reference of EVERY call starts from the cache as the device holds it before that call (cache.values()): a call is judged for what it does,
by its own class, and not for the roundings its predecessors left in the cache - which, under the rows kernel's atomics, differ from run to run.
What a follow-up call adds to the first call's state and slot checks is therefore this: it reads what was really stored, where it was stored.

Operative matrix form per (weight set, regime), from the descriptor comments of include/vv_hip.h and from weights.py (_mat_q: the bf16 copy of
a matrix that has a companion holds the companion's EFFECTIVE values, exact in bf16 in every format, so every form of one matrix holds the same
numbers and the reference is handed effective_state_dict's matrix whatever form the table names; a loop that read a matrix the set does not
have would read NULL).  Which form is READ is pinned on the device through the vv_linear profiler (vv_prof_begin / vv_prof_end record the weight
type of every vv_linear launch, and of the rows launches under VV_WQ_FRAG4 / VV_WQ_FRAG6):

  set \\ regime        1..2 rows           decode 3..8         decode 9..16        decode 17+, prompt 3..63    prompt >= 64
  fp32                fp32                fp32                fp32                fp32                        fp32
  bf16                bf16                bf16 (rows kernel)  bf16 (mfma)         bf16 (gemv <= 8, mfma)      bf16 (prefill branch)
  bf16_frag           bf16                fragment copy       fragment copy (16)  bf16                        bf16
  fp8                 fp8 companion       bf16 (rows kernel)  bf16 (mfma)         bf16                        bf16
  fp8_frag            fp8 companion       fp8 fragment codes  bf16 (mfma)         bf16                        bf16
  nf4                 NF4 companion       bf16 (rows kernel)  bf16 (mfma)         bf16                        bf16
  mxfp4 / mxfp6       MX companion        bf16 (rows kernel)  bf16 (mfma)         bf16                        bf16
  *_row_batch         MX companion        MX fragment codes   bf16 (mfma)         bf16                        bf16
  *_lean              MX companion        refused             refused             codes (GEMM on the codes)   codes (GEMM on the codes)
Limit of that pin: the profiler records the rows kernel's launches only under VV_WQ_FRAG4 / VV_WQ_FRAG6 (include/vv_hip.h).  For decode at 3..8
rows on bf16, bf16_frag, fp8, fp8_frag, nf4 and the plain mx sets, and for bf16_frag at 9..16, expected_forms can only require that NO vv_linear
launch shows another weight type; "fragment copy", "fp8 fragment codes" and "bf16 (rows kernel)" of the table are asserted by nothing here - since
all forms hold the same numbers, a loop that fed the bf16 matrix where the table says fragment copy would pass.  tests/test_hip_gemv.py and
tests/test_hip_gemv_rows16.py pin those operand forms at the kernel.

Cases (CASES below): name -> branch.  Every call is followed by at least one more on the same cache.
  dec_r1, dec_r2 (every set)            decode, streaming GEMVs on the companion / matrix        dec_r2_ldx: ldx > hidden, NaN in the pitch gap
  dec_r3 / r4 / r8 (+ _frag, fp8, mx)   rows8: vv_copy_rows into h, split-K workspace            dec_r2_long: s_max 1088 > 1024, att_split 3, tickets memset
  dec_r9 / r16 _frag                    rows16                                                   dec_r9 / r16 (no copies): the generic linears (mfma)
  dec_r17                               past both attention row caps                             dec_*_f32: the fp32 model
  pre_r1, pre_r5, pre_r16               prompt rows, 16 = first R of the matrix-core attention   pre_r63 / pre_r64: either side of VV_PREFILL_ROWS
  pre_r150                              crosses a 128-row tile                                   pre_chunked: two calls, the second at pos0 = 40
  pre_mixed                             rows of three cache rows in mixed order                  packed_mixed: the same through vv_llm_prefill_packed,
  lean_r3 / lean_r64                    the GEMM on the codes                                      sel of 3 rows, vv_tune("gemm_packed_rows", 64)
  *_B                                   geometry B                                               dec_r2_nonorm: out == NULL, ws starts with pre-norm h
  kv8_r2_bf16 (test_decode_on_an_fp8_cache_vs_fp64): two prompts into a bf16 cache, vv_kv_quantize, two decode steps of R = 2 on the fp8 cache at
                                        s_max 1088: vv_attn_decode_ws appending to an fp8 cache from inside the loop, att_split 3, tickets memset

Compared per call: every output row against its reference row (global, worst row, worst element); K and V of every touched (layer, cache row,
slot) against the reference cache; vt == vt_tiles(v) exactly; every other slot keeps its bits; x, lens, cache_rows and all parameters are
bit-unchanged; two runs into separate caches are bit-identical (the rows kernel adds split-K slices with fp32 atomics under gemv_rows_atomic: held
to the bar only, as in tests/test_hip_gemv.py).  The workspace holds exactly vv_llm_ws_bytes(m, R) bytes of 0xFF between two 0xFF guards of the
same size (>= the largest carve), both intact afterwards.

Bars (BAR), one per class, by the house rule of test_hip_conv_stream.py: >= 8 x the CPU stand-in's error against the fp64 reference (run_llm in
fp32 with the class's rounding of every linear's activations: none, bf16 hi + lo, bf16), <= 1/10 of the cost of each fault (a)..(i) of FAULTS put
into the stand-in, on the figure meant to catch it; test_bars_sit_between_floor_and_faults holds both, JUDGED_ELSEWHERE lists the (class, fault)
pairs whose cost leaves no room, exact in both directions.  The decode step on an fp8 cache has the dec class's output bar and a state bar of
its own ("state kv8").

Measured on the MI355X, one run of the whole file (profiles/llm_loop_parity.txt holds the same table and every call), largest value over the
class's calls:
  class       comparisons  figure    bar       largest     bar / largest   where
  fp32        10           out       2.0e-05   5.962e-07   33.5            dec_r9_fp32 call 0
  fp32        10           element   1.2e-04   2.819e-06   42.6
  dec         73           out       1.0e-04   7.051e-07   141.8           kv8_r2_bf16 call 2
  dec         73           element   6.0e-04   3.398e-06   176.6
  rows        50           out       3.0e-04   3.581e-06   83.8            dec_r9_bf16_frag_B call 0
  rows        50           element   1.8e-03   1.898e-05   94.8
  pre         24           out       2.5e-02   3.078e-03   8.1             pre_r16_bf16 call 0
  pre         24           element   1.5e-01   2.561e-02   5.9
  state fp32  10           state     2.0e-05   5.917e-07   33.8            dec_r9_fp32 call 1
  state dec   71           state     5.0e-03   1.523e-05   328.3           dec_r2_long_bf16 call 0
  state kv8   2            state     1.7e-02   0.000e+00   -
  state rows  50           state     5.0e-03   1.008e-03   5.0             dec_r4_mxfp6 call 1
  state pre   24           state     3.0e-02   4.027e-03   7.4             pre_mixed_bf16 call 0
Within a factor of ten of their bars: pre out (8.1 x), pre element (5.9 x), state pre (7.4 x) and state rows (5.0 x).  pre is the bf16 rounding of
the activations itself: the stand-in's floor is 2.8e-3 / 1.5e-2 / 3.7e-3, so the device adds nothing to speak of.  state rows: the rows kernel's
hi + lo operand (2^-17) moves a few stored values across a bf16 rounding edge per call; the stand-in shows the same 5e-4.  state kv8 is 0: both
decode steps appended exactly the reference's codes.
"""
import ctypes as C
import dataclasses
import functools
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_rms, vt_tiles
from test_hip_attn_decode import _angle, _rot64, ref_decode_fp64
from test_hip_attn_prefill import ref_prompt_fp64, ref_rope_store_fp64
from test_hip_kv_fp8 import _codes as fp8_codes, _scale_rule as fp8_scale_rule

gpu = pytest.mark.gpu
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
VV_E_ARG, VV_E_HIP, VV_E_UNSUPPORTED = -1, -2, -3
SENTINEL = 77.0            # exact in bf16; fills every cache slot no row owns
SENT32 = 0x7FC0BEEF        # NaN: pitch gaps, guard rows of out
FLOOR_HEADROOM, FAULT_MARGIN = 8, 10
ELEM = 6                   # element bar = ELEM x the class bar (the largest of up to 150 x 512 near-normal errors is about 4.5 sigma)

# one constant per class: out figures (global, worst row; ELEM x for the worst element) and the state figure (worst touched K / V slot)
# state, bf16 cache: fp32-sized noise moves a stored value across a rounding edge now and then, and ONE such flip (2^-8 of an element up to 4 rms
# large, in a vector of 256) costs its slot up to 1e-3: the bar leaves room for a few
# state, fp8 cache (kv8): an e4m3 code has 3 mantissa bits, so ONE flip costs 2^-4 of an element up to 4 rms large in a vector of 256: 1.6e-2
BAR = {"fp32": 2e-5, "dec": 1e-4, "rows": 3e-4, "pre": 2.5e-2, "state fp32": 2e-5, "state dec": 5e-3, "state rows": 5e-3, "state pre": 3e-2,
       "state kv8": 1.7e-2}
FAULTS = {"a": "layer-0 residual read at pitch hidden instead of ldx", "b": "one row's RoPE position off by one",
          "c": "K / V stored one slot late", "c2": "K / V stored on the neighbouring cache row", "d": "attention over lens[r] keys instead of lens[r] + 1",
          "e": "the qkv bias dropped", "f": "ln1 used for ln2", "g": "the down-projection residual dropped in layer 1",
          "h": "the final norm on row sel[i] + 1", "i": "the bf16 matrix of the unquantised weights where the table says companion"}
# (class, fault) pairs whose cost to the figure meant to catch them is below 10 x the class bar, exact in both directions.  (pre, b): one position
# of RoPE moves a stored K by 0.21 rel RMS, and a K that follows activations rounded to bf16 already differs by 3.5e-3 from fp64; the rotation and
# the position of the store are pinned at 4e-3 by group E of tests/test_hip_attn_prefill.py and of tests/test_hip_attn_decode.py, and the loop
# hands every class the same rope table and lens
JUDGED_ELSEWHERE = {("pre", "b")}


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
# models and weights (CPU)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cfg_of(geom):
    from vibevoice_rocm_amd.config import VVConfig
    return dataclasses.replace(VVConfig.preset("mid"), layers=2, vocab=64, head_layers=1, heads=4 if geom == "A" else 12)


@functools.lru_cache(maxsize=None)
def sd_of(geom):
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    sd = synth_state_dict_torch(cfg_of(geom), 4242, device="cpu")
    for k in sd:
        if k.endswith(("q_proj.bias", "k_proj.bias", "v_proj.bias")):
            sd[k] = sd[k] * 20
        if k.startswith(LLM) and k.endswith(("layernorm.weight", "norm.weight")):
            sd[k] = 1 + 5 * (sd[k] - 1)
    return sd


# weight set -> (torch dtype, weight_quant, DeviceWeights keywords, ensure_frag)
SETS = {"fp32": (F32, None, {}, False), "bf16": (BF16, None, {}, False), "bf16_frag": (BF16, None, {}, True),
        "fp8": (BF16, "fp8", {}, False), "fp8_frag": (BF16, "fp8", {}, True), "nf4": (BF16, "nf4", {}, False),
        "mxfp4": (BF16, "mxfp4", {}, False), "mxfp4_row_batch": (BF16, "mxfp4", {"mxfp4_row_batch": True}, True), "mxfp4_lean": (BF16, "mxfp4", {"mxfp4_lean": True}, False),
        "mxfp6": (BF16, "mxfp6", {}, False), "mxfp6_row_batch": (BF16, "mxfp6", {"mxfp6_row_batch": True}, True), "mxfp6_lean": (BF16, "mxfp6", {"mxfp6_lean": True}, False)}
LLM = "model.language_model."


@functools.lru_cache(maxsize=None)
def ref_weights(geom, wset, unquantised=False):
    """the LLM's parameters as the device holds them, fp32 tensors: fp32 as drawn; bf16 widened exactly; a quantised set's matrices are
    effective_state_dict's (unquantised=True: fault (i), the bf16 rounding of the matrix as drawn)"""
    from vibevoice_rocm_amd.weights import effective_state_dict
    cfg, sd = cfg_of(geom), sd_of(geom)
    dt, quant, _, _ = SETS[wset]
    src = effective_state_dict(cfg, sd, quant) if quant and not unquantised else sd
    mat = (lambda t: t.float()) if dt == F32 else (lambda t: t.to(BF16).float())
    layers = []
    for l in range(cfg.layers):
        p = f"{LLM}layers.{l}."
        cat = lambda s, kind: torch.cat([s[p + f"self_attn.{n}_proj.{kind}"] for n in "qkv"], 0)
        layers.append(dict(ln1=sd[p + "input_layernorm.weight"], ln2=sd[p + "post_attention_layernorm.weight"], wqkv=mat(cat(src, "weight")),
                           bqkv=cat(sd, "bias").float(), wo=mat(src[p + "self_attn.o_proj.weight"]), wgate=mat(src[p + "mlp.gate_proj.weight"]),
                           wup=mat(src[p + "mlp.up_proj.weight"]), wdown=mat(src[p + "mlp.down_proj.weight"])))
    inv_freq = 1.0 / (cfg.rope_theta ** (torch.arange(0, cfg.head_dim, 2, dtype=torch.float) / cfg.head_dim))
    return dict(cfg=cfg, layers=layers, final_norm=sd[LLM + "norm.weight"], inv_freq=inv_freq)


# ---------------------------------------------------------------------------------------------------------------
# the reference (and, with dtype / rnd / fault, the CPU stand-in)
# ---------------------------------------------------------------------------------------------------------------
def new_cache(cfg, rows, s_max, dtype=BF16):
    """k, v [layers, rows, kv_heads, s_max, d] fp64 tensors that hold cache-type-exact values; every slot starts as SENTINEL"""
    shape = (cfg.layers, rows, cfg.kv_heads, s_max, cfg.head_dim)
    rnd = (lambda t, l=None, which=None: t.float().to(BF16).double()) if dtype == BF16 else (lambda t, l=None, which=None: t.float().double())
    return dict(k=torch.full(shape, SENTINEL, dtype=F64), v=torch.full(shape, SENTINEL, dtype=F64), rnd=rnd, dtype=dtype)


def fill_cache(cache, lens, seed):
    """slots [0, lens[r]) of cache row r: random cache-type-exact values (what earlier steps left)"""
    g = torch.Generator().manual_seed(seed)
    for r, n in enumerate(lens):
        if n:
            shape = (cache["k"].shape[0], cache["k"].shape[2], n, cache["k"].shape[4])
            cache["k"][:, r, :, :n] = cache["rnd"](torch.randn(shape, generator=g))
            cache["v"][:, r, :, :n] = cache["rnd"](torch.randn(shape, generator=g))


F8 = torch.float8_e4m3fn


def fp8_values(codes, scale):
    """the values an fp8 cache holds: fp32(code) * scale of its (layer, KV head); codes [layers, rows, kv_heads, s_max, d] uint8, scale [layers, kv_heads]"""
    return (codes.view(F8).float() * scale[:, None, :, None, None]).double()


def quantize_cache(cache, lens):
    """vv_kv_quantize restated with the helpers of tests/test_hip_kv_fp8.py: the scales of every (layer, KV head) from the absmax of cache row 0
    over its filled slots (VV_KVQ_DERIVE_SCALES), then slots [0, lens[r]) of every row as saturating e4m3 codes under them.  The cache becomes an
    fp8 cache: it holds code * scale, and a decode step appends its new k / v rounded the same way.  Returns (k codes, v codes, kscale, vscale)."""
    out = {}
    for which in ("k", "v"):
        t = cache[which]
        sc = fp8_scale_rule(t[:, 0, :, : lens[0]].abs().amax((-1, -2)))              # [layers, kv_heads]
        codes = fp8_codes(t, sc[:, None, :, None, None])
        filled = torch.zeros_like(codes, dtype=torch.bool)
        for r, n in enumerate(lens):
            filled[:, r, :, :n] = True
        codes = torch.where(filled, codes, torch.full_like(codes, FP8_SENTINEL))
        out[which], out[which + "scale"] = codes, sc
        cache[which] = fp8_values(codes, sc)
    ks, vs = out["kscale"], out["vscale"]
    cache["rnd"] = lambda t, l, which: (fp8_codes(t, (ks if which == "k" else vs)[l][:, None]).view(F8).float() * (ks if which == "k" else vs)[l][:, None]).double()
    cache["dtype"] = F8
    return out["k"], out["v"], ks, vs


FP8_SENTINEL = 0x48        # the e4m3 code that fills every slot of an fp8 cache no row owns (a finite value)


def _rms(x, w, eps):
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + eps) * w.to(x.dtype)


def run_llm(W, x, positions, cache_rows, cache, dtype=F64, rnd=None, fault=None, sel=None, final_norm=True):
    """R rows x[R, >= hidden] (columns past hidden are a pitch gap) at positions[r] of cache row cache_rows[r] (None: the decode step, row r on
    cache row r) through the decoder stack; appends to cache; returns the final-normed rows (sel: those rows only; final_norm=False: the
    pre-norm hidden state).  fp64 and no rounding: the reference.  dtype=fp32 with rnd (applied to every linear's activations): the stand-in.
    fault: one of FAULTS, put into the stand-in for the bar test."""
    cfg = W["cfg"]
    H, nh, nkv, d, eps = cfg.hidden, cfg.heads, cfg.kv_heads, cfg.head_dim, cfg.rms_eps
    R = x.shape[0]
    lens = [int(p) for p in positions]
    crows = list(range(R)) if cache_rows is None else [int(c) for c in cache_rows]
    rnd = rnd if isinstance(rnd, dict) else {s: rnd for s in SITES}

    def lin(site, t, w, b=None):
        t = rnd[site](t) if rnd.get(site) else t
        return F.linear(t, w.to(dtype), None if b is None else b.to(dtype))
    h = x[:, :H].to(dtype)
    res0 = x.reshape(-1)[: R * H].view(R, H).to(dtype) if fault == "a" else h
    inv_freq = W["inv_freq"]
    for l, Lw in enumerate(W["layers"]):
        qkv = lin("qkv", _rms(h, Lw["ln1"], eps), Lw["wqkv"], None if fault == "e" else Lw["bqkv"])
        if fault == "b":                        # the middle row rotated one position further: R(pos + 1) = R(1) R(pos)
            q1 = qkv.double().clone()
            one = _angle(1, inv_freq)
            q1[R // 2, : (nh + nkv) * d] = _rot64(q1[R // 2, : (nh + nkv) * d].view(nh + nkv, d), one).reshape(-1)
            qkv = q1.to(dtype)
        kc, vc = cache["k"][l], cache["v"][l]
        slot = [n + 1 if fault == "c" else n for n in lens]
        srow = [min(c + 1, kc.shape[0] - 1) if fault == "c2" else c for c in crows]
        if cache_rows is None and fault != "d":
            att, kn, vn = ref_decode_fp64(qkv, kc, vc, lens, inv_freq, nh)
            for r in range(R):
                kc[srow[r], :, slot[r]], vc[srow[r], :, slot[r]] = cache["rnd"](kn[r], l, "k"), cache["rnd"](vn[r], l, "v")
        else:
            q, kn, vn = ref_rope_store_fp64(qkv, lens, inv_freq, nh, nkv, d)
            for r in range(R):
                kc[srow[r], :, slot[r]], vc[srow[r], :, slot[r]] = cache["rnd"](kn[r], l, "k"), cache["rnd"](vn[r], l, "v")
            alens = [max(n - 1, 0) for n in lens] if fault == "d" else lens
            att = ref_prompt_fp64(q, kc, vc, alens, crows, nh)
        h = (res0 if l == 0 else h) + lin("o", att.reshape(R, nh * d).to(dtype), Lw["wo"])
        n2 = _rms(h, Lw["ln1"] if fault == "f" else Lw["ln2"], eps)
        act = F.silu(lin("gate_up", n2, Lw["wgate"])) * lin("gate_up", n2, Lw["wup"])
        down = lin("down", act, Lw["wdown"])
        h = down if (fault == "g" and l == 1) else h + down
    if not final_norm:
        return h.double()
    rows = list(range(R)) if sel is None else [int(s) for s in sel]
    if fault == "h":
        rows = [(s + 1) % R for s in rows]
    return _rms(h[rows], W["final_norm"], eps).double()


def rnd_bf16(t):
    return t.to(BF16).to(t.dtype)


def rnd_hilo(t):
    """the rows kernel's activation operand: bf16 hi + bf16 lo"""
    hi = t.to(BF16).to(t.dtype)
    return hi + (t - hi).to(BF16).to(t.dtype)


SITES = ("qkv", "o", "gate_up", "down")


def _route(m, n, k, wdt, pro=False, bias=False, res=False, dual=False):
    """the kernel vv_linear takes for one of the loop's linears outside the rows kernel and the prefill branch.  Host only."""
    L, l = _lib()
    a = L.LinArgs()
    a.x, a.ldx, a.m, a.pro, a.eps = 0x10000, k, m, (L.PRO_RMSNORM if pro else L.PRO_NONE), 1e-6
    a.norm_w = 0x20000 if pro else None
    a.bias = 0x40000 if bias else None
    a.w, a.n, a.k, a.wdt, a.out, a.ldo = 0x30000, n, k, wdt, 0x50000, n
    if dual:
        a.w2, a.act = 0x80000, L.ACT_SWIGLU
    if res:
        a.res, a.ldres = 0x60000, n
    buf = C.create_string_buffer(128)
    L.check(l.vv_linear_route(C.byref(a), buf, 128), "vv_linear_route")
    return buf.value.decode()


def site_routes(geom, R, wdt=1):
    cfg = cfg_of(geom)
    H, qd, qkvd, I = cfg.hidden, cfg.heads * cfg.head_dim, (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim, cfg.inter
    return {"qkv": _route(R, qkvd, H, wdt, pro=True, bias=True), "o": _route(R, H, qd, wdt, res=True),
            "gate_up": _route(R, I, H, wdt, pro=True, dual=True), "down": _route(R, H, I, wdt, res=True)}


@functools.lru_cache(maxsize=None)
def klass_of(geom, wset, R, decode):
    """(class, stand-in rounding) of a call: the class names the bar that judges it.
      fp32   fp32 weights: no rounding anywhere
      rows   the rows kernel (decode, 3..8 rows of a bf16-typed set; 9..16 with bf16 fragment copies): activations as bf16 hi + lo
      pre    activations rounded to bf16 once in front of a linear: the prefill branch (>= 64 rows; a lean set's prompt rows from 3 on) at all
             four linears, else at the linears for which vv_linear_route names a matrix-core kernel (mfma_*, skinny)
      dec    everything else: fp32 activations on bf16-exact weights"""
    if wset == "fp32":
        return "fp32", None
    if decode and (3 <= R <= 8 or (9 <= R <= 16 and wset == "bf16_frag")):
        return "rows", rnd_hilo
    if R >= 64 or (wset.endswith("_lean") and not decode and R >= 3):
        return "pre", rnd_bf16
    if R <= 2:
        return "dec", None
    rounds = {s: (rnd_bf16 if name.startswith(("mfma_", "skinny")) else None) for s, name in site_routes(geom, R).items()}
    return ("pre" if any(rounds.values()) else "dec"), rounds


def figures(got, ref):
    """(global rel RMS, worst row rel RMS, worst element as |err| / rms(ref row)); a non-finite got gives inf"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.where(np.isfinite(got), got - ref, np.inf)
    rms = np.sqrt((ref ** 2).mean(-1))
    with np.errstate(over="ignore", invalid="ignore"):
        return (float(np.sqrt((err ** 2).mean()) / np.sqrt((ref ** 2).mean())), float((np.sqrt((err ** 2).mean(-1)) / rms).max()),
                float((np.abs(err).max(-1) / rms).max()))


def touched_slots(cfg, lens, crows):
    return [(c, n) for n, c in zip(lens, crows)]


def state_figure(got_k, got_v, ref_k, ref_v, slots):
    """worst rel RMS over the touched (layer, cache row, slot) vectors [kv_heads * d] of K and of V"""
    worst = 0.0
    for g, r in ((got_k, ref_k), (got_v, ref_v)):
        for c, n in slots:
            a, b = g[:, c, :, n].double().reshape(g.shape[0], -1).numpy(), r[:, c, :, n].double().reshape(r.shape[0], -1).numpy()
            err = np.where(np.isfinite(a), a - b, np.inf)
            with np.errstate(over="ignore", invalid="ignore"):
                worst = max(worst, float((np.sqrt((err ** 2).mean(-1)) / np.sqrt((b ** 2).mean(-1))).max()))
    return worst


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
LENS = [0, 33, 31, 32, 5, 64, 1, 40, 63, 2, 65, 30, 34, 7, 0, 31, 32]      # unequal; 0, and either side of the 32- and 64-key tile edges


def _dec(R, n_calls=2, **kw):
    """a decode case: R rows on R cache rows whose first lens[r] slots are filled; call i runs at lens + i"""
    lens = kw.pop("lens", LENS[:R])
    return dict(kind="dec", rows=R, s_max=kw.pop("s_max", 96), fill=lens, calls=[dict(R=R, lens=[n + i for n in lens], crows=None, **kw) for i in range(n_calls)])


def _pre(R, pos0=0, rows=2, crow=1, then=True, **kw):
    """a prompt case: R rows at pos0.. of one cache row, then one more prompt row behind them and (bf16) a decode step on all cache rows"""
    s_max = -(-(pos0 + R + 3) // 32) * 32
    calls = [dict(R=R, lens=list(range(pos0, pos0 + R)), crows=[crow] * R, **kw)]
    if then:
        calls.append(dict(R=1, lens=[pos0 + R], crows=[crow]))
    return dict(kind="pre", rows=rows, s_max=s_max, fill=[pos0 if r == crow else 0 for r in range(rows)], calls=calls)


def _mixed_rows(counts=(23, 19, 26), seed=5):
    """rows of three cache rows in mixed order: each cache row's positions ascend from 0, the cache rows follow each other at random"""
    g = torch.Generator().manual_seed(seed)
    order = torch.tensor([c for c, n in enumerate(counts) for _ in range(n)])[torch.randperm(sum(counts), generator=g)].tolist()
    nxt, lens = [0, 0, 0], []
    for c in order:
        lens.append(nxt[c])
        nxt[c] += 1
    return dict(lens=lens, crows=order)


MIXED = _mixed_rows()


def _mixed(packed):
    R = len(MIXED["lens"])
    last = {c: max(n for n, cc in zip(MIXED["lens"], MIXED["crows"]) if cc == c) for c in (0, 1, 2)}
    first = dict(R=R, lens=MIXED["lens"], crows=MIXED["crows"])
    if packed:
        first.update(packed=True, sel=[max(i for i in range(R) if MIXED["crows"][i] == c) for c in (1, 2, 0)])
    return dict(kind="pre", rows=3, s_max=32, fill=[0, 0, 0], calls=[first, dict(R=3, lens=[last[c] + 1 for c in (0, 1, 2)], crows=None)])


def _cases():
    c = {}
    for s in SETS:
        for R in (1, 2):
            c[f"dec_r{R}_{s}"] = dict(_dec(R), wset=s)
    c["dec_r2_ldx_bf16"] = dict(_dec(2, ldx_pad=8), wset="bf16")
    c["dec_r2_long_bf16"] = dict(_dec(2, lens=[1030, 700], s_max=1088), wset="bf16")
    c["dec_r2_nonorm_bf16"] = dict(_dec(2, out_null=True), wset="bf16")
    for R in (3, 4, 8):
        for s in ("bf16", "bf16_frag", "fp8", "fp8_frag", "nf4", "mxfp4", "mxfp4_row_batch", "mxfp6", "mxfp6_row_batch"):
            if R == 4 or s in ("bf16", "bf16_frag", "fp8_frag", "mxfp4_row_batch", "mxfp6_row_batch"):
                c[f"dec_r{R}_{s}"] = dict(_dec(R), wset=s)
    for R in (9, 16):
        c[f"dec_r{R}_bf16_frag"] = dict(_dec(R), wset="bf16_frag")
        c[f"dec_r{R}_bf16"] = dict(_dec(R), wset="bf16")
    c["dec_r17_bf16"] = dict(_dec(17), wset="bf16")
    for R in (3, 9):
        c[f"dec_r{R}_fp32"] = dict(_dec(R), wset="fp32")
    for R in (1, 5, 16, 63, 64, 150):
        c[f"pre_r{R}_bf16"] = dict(_pre(R), wset="bf16")
    c["pre_r5_fp32"] = dict(_pre(5), wset="fp32")
    c["pre_r64_fp8"] = dict(_pre(64), wset="fp8")
    chunked = _pre(37, pos0=40)
    chunked.update(fill=[0, 0], calls=[dict(R=40, lens=list(range(40)), crows=[1] * 40)] + chunked["calls"])
    c["pre_chunked_bf16"] = dict(chunked, wset="bf16")
    c["pre_mixed_bf16"] = dict(_mixed(False), wset="bf16")
    c["packed_mixed_bf16"] = dict(_mixed(True), wset="bf16")
    for s in ("mxfp4_lean", "mxfp6_lean"):
        c[f"lean_r3_{s}"] = dict(_pre(3), wset=s)
        c[f"lean_r64_{s}"] = dict(_pre(64), wset=s)
    # geometry B: bf16 and one lean format
    for name in ("dec_r2_bf16", "dec_r4_bf16", "dec_r4_bf16_frag", "dec_r9_bf16_frag", "pre_r16_bf16", "pre_r64_bf16", "lean_r64_mxfp6_lean", "dec_r2_mxfp6_lean"):
        c[name + "_B"] = dict(c[name], geom="B", wset=c[name]["wset"])
    for v in c.values():
        v.setdefault("geom", "A")
    return c


CASES = _cases()


def case_x(name, i, R, H, pad):
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{i}".encode()))
    x = torch.zeros(R, H + pad)
    x[:, :H] = torch.randn(R, H, generator=g)
    return x


def initial_cache(name):
    """the cache a case starts from (fp64 tensors of cache-type-exact values): slots [0, fill[r]) random, SENTINEL elsewhere"""
    case = CASES[name]
    cache = new_cache(cfg_of(case["geom"]), case["rows"], case["s_max"], F32 if case["wset"] == "fp32" else BF16)
    fill_cache(cache, case["fill"], zlib.crc32(name.encode()))
    return cache


# ---------------------------------------------------------------------------------------------------------------
# CPU tests: the reference against the oracle, the classes against the routes, the bars
# ---------------------------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_oracle():
    """run_llm in fp32 on an fp32 cache against oracle.vv_oracle.llm_forward: a 21-row prompt on cache row 1, then three decode steps"""
    from oracle import vv_oracle as O
    W = ref_weights("A", "fp32")
    cfg, sd = W["cfg"], sd_of("A")
    g = torch.Generator().manual_seed(3)
    kv = O.KVCache(cfg.layers)
    cache = new_cache(cfg, 2, 32, F32)
    x = torch.randn(21, cfg.hidden, generator=g)
    want = O.llm_forward(sd, cfg.as_dict(), x, kv, 0)
    got = run_llm(W, x, range(21), [1] * 21, cache, dtype=F32)
    assert rel_rms(got.numpy(), want.double().numpy(), "run_llm fp32 vs O.llm_forward, prompt (CPU)") < 2e-6
    for step in range(3):
        x = torch.randn(1, cfg.hidden, generator=g)
        want = O.llm_forward(sd, cfg.as_dict(), x, kv, 21 + step)
        # the decode convention on cache row 0 needs the prompt there: move it once
        if step == 0:
            cache["k"][:, 0], cache["v"][:, 0] = cache["k"][:, 1].clone(), cache["v"][:, 1].clone()
        got = run_llm(W, x, [21 + step], None, cache, dtype=F32)
        assert rel_rms(got.numpy(), want.double().numpy(), f"run_llm fp32 vs O.llm_forward, decode step {step} (CPU)") < 2e-6
    k_or = torch.stack([kv.k[l] for l in range(cfg.layers)])          # [layers, kvh, S, d]
    assert rel_rms(cache["k"][:, 0, :, :24].numpy(), k_or.double().numpy(), "run_llm cache K vs the oracle's (CPU)") < 2e-6


def test_classes_match_the_routes():
    """what klass_of rests on: every route of the loop's linears at the row counts of the cases is a gemv (fp32 activations), the fp32 GEMM, or a
    matrix-core kernel that rounds the activations to bf16 once; fp32 weights never meet the latter; and the classes of the cases are the ones the
    bar study covers"""
    for geom in "AB":
        for R in (3, 5, 8, 9, 16, 17, 63):
            for site, name in site_routes(geom, R).items():
                assert name.startswith(("gemv_", "gemm_f32", "mfma_", "skinny")), (geom, R, site, name)
            for site, name in site_routes(geom, R, 0).items():
                assert name.startswith(("gemv_", "gemm_f32")), (geom, R, site, name)
    assert klass_of("A", "bf16", 64, False)[0] == "pre" and klass_of("A", "mxfp4_lean", 3, False)[0] == "pre" and klass_of("A", "bf16", 8, True)[0] == "rows"
    assert klass_of("A", "bf16", 9, True)[0] == "pre" and klass_of("A", "bf16", 17, True)[0] == "pre" and klass_of("A", "fp8", 2, False)[0] == "dec"
    seen = {klass_of(c["geom"], c["wset"], call["R"], call["crows"] is None)[0] for c in CASES.values() for call in c["calls"]}
    assert seen == {"fp32", "dec", "rows", "pre"}, seen


def _chain(R, pos, crows, sel=None):
    """a call and its follow-up: the decode step again one position on, or one more prompt row behind the prompt"""
    pos = list(pos)
    first = dict(R=R, lens=pos, crows=crows, sel=sel)
    if crows is None:
        return [first, dict(R=R, lens=[n + 1 for n in pos], crows=None, sel=None)]
    return [first, dict(R=1, lens=[pos[-1] + 1], crows=[crows[0]], sel=None)]


def _fault_runs(klass):
    """(tag, weight set, geom, chain, faults) of the bar study for a class; the FIRST call of a chain has the class, a follow-up its own"""
    every = list("abcdefgh") + ["c2"]
    if klass in ("dec", "fp32"):
        s = "bf16" if klass == "dec" else "fp32"
        return [("decode R=2", s, "A", _chain(2, [33, 5], None), every), ("prompt R=5", s, "A", _chain(5, range(7, 12), [1] * 5, [0, 2, 3]), every),
                ("decode R=2 fp8", "fp8", "A", _chain(2, [33, 5], None), ["i"])][: 3 if klass == "dec" else 2]
    if klass == "kv8":
        return [("decode R=2 on an fp8 cache", "bf16", "A", _chain(2, [40, 33], None), list("bcdefgh"))]
    if klass == "rows":
        return [("decode R=4", "bf16", "A", _chain(4, [0, 33, 31, 32], None), every), ("decode R=8", "bf16", "B", _chain(8, LENS[:8], None), every)]
    return [("prompt R=64", "bf16", "A", _chain(64, range(3, 67), [1] * 64, [0, 32, 62]), every), ("decode R=9 mfma", "bf16", "A", _chain(9, LENS[:9], None), every),
            ("prompt R=16", "bf16", "B", _chain(16, range(16), [1] * 16), every)]


def _copy_cache(c):
    return dict(c, k=c["k"].clone(), v=c["v"].clone())


@pytest.mark.parametrize("klass", ["fp32", "dec", "kv8", "rows", "pre"])
def test_bars_sit_between_floor_and_faults(klass):
    """condition 1: each bar >= 8 x the stand-in's figures against the fp64 reference; condition 2: each bar <= 1/10 of the cost of every fault to
    the figure meant to catch it - the worst output row, or for (b), (c), (c2) the state figure (a wrongly rotated or misplaced K is what
    the cache holds, whatever the call's own output makes of it).  Both over a call and its follow-up on the same cache, the fault in both;
    as on the device, the reference of a call starts from the cache the run under test holds before it.  kv8 is the decode step on an fp8 cache:
    its outputs are the dec class's, its state figure has a bar of its own.  A pair that cannot meet condition 2 must be in JUDGED_ELSEWHERE,
    and a pair listed there without need fails too."""
    elsewhere = set()
    for tag, wset, geom, chain, letters in _fault_runs(klass):
        W = ref_weights(geom, wset)
        cfg = W["cfg"]
        kvdt = F32 if wset == "fp32" else BF16
        decode = chain[0]["crows"] is None
        kout = "dec" if klass == "kv8" else klass
        kst = "state " + klass
        assert klass_of(geom, wset, chain[0]["R"], decode)[0] == kout, tag

        def run(W=W, fault=None):
            """per call of the chain the stand-in's figures against the reference that starts from the stand-in's cache: (out, element, state, row)"""
            cache = new_cache(cfg, chain[0]["R"] if decode else 3, 96, kvdt)
            fill_cache(cache, chain[0]["lens"] if decode else [0, chain[0]["lens"][0], 0], 11)
            if klass == "kv8":
                quantize_cache(cache, chain[0]["lens"])
            res = []
            for i, call in enumerate(chain):
                x = case_x("bars" + tag, i, call["R"], cfg.hidden, 8)
                ref_cache = _copy_cache(cache)
                want = run_llm(ref_weights(geom, wset), x.double(), call["lens"], call["crows"], ref_cache, sel=call["sel"])
                if fault == "a":
                    x[:, cfg.hidden:] = 1.0                # the gap holds NaN on the device; a finite value shows the smaller cost
                y = run_llm(W, x.float(), call["lens"], call["crows"], cache, sel=call["sel"], dtype=F32, fault=fault,
                            rnd=klass_of(geom, wset, call["R"], call["crows"] is None)[1])
                o = figures(y, want)
                st = state_figure(cache["k"], cache["v"], ref_cache["k"], ref_cache["v"], touched_slots(cfg, call["lens"], range(call["R"]) if call["crows"] is None else call["crows"]))
                res.append((max(o[:2]), o[2], st, o[1]))
            return [max(r[j] for r in res) for j in range(4)]
        f_out, f_el, f_st, _ = run()
        print(f"{klass} {tag}: stand-in floor out {f_out:.2e} element {f_el:.2e} state {f_st:.2e}  (bars {BAR[kout]:.1e} / {BAR[kst]:.1e})")
        assert BAR[kout] >= FLOOR_HEADROOM * f_out and ELEM * BAR[kout] >= FLOOR_HEADROOM * f_el and BAR[kst] >= FLOOR_HEADROOM * f_st, (tag, f_out, f_el, f_st)
        for f in letters:
            kw = dict(W=ref_weights(geom, wset, unquantised=True)) if f == "i" else dict(fault=f)
            _, _, c_st, c_out = run(**kw)
            on_state = f in ("b", "c", "c2")
            cost, bar = (c_st, BAR[kst]) if on_state else (c_out, BAR[kout])
            print(f"{klass} {tag}: fault ({f}) costs out {c_out:.2e} state {c_st:.2e}  judged on {'state' if on_state else 'out'}")
            if not bar <= cost / FAULT_MARGIN:
                elsewhere.add((klass, f))
    print(f"{klass}: judged elsewhere: {sorted(elsewhere)}")
    assert elsewhere == {p for p in JUDGED_ELSEWHERE if p[0] == klass}, sorted(elsewhere)


# ---------------------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------------------
_DW = {}
WQ_CODE = {"fp8": 2, "nf4": 3, "mxfp4": 4, "mxfp6": 6}       # VV_FP8, VV_NF4, VV_MXFP4, VV_MXFP6
FRAG_CODE = {"mxfp4": 5, "mxfp6": 8}                          # VV_MXFP4_FRAG, VV_MXFP6_FRAG


def device_weights(geom, wset, device="cuda"):
    """the package's DeviceWeights for a weight set (built once per process), and bit copies of every tensor it owns"""
    key = (geom, wset, device)
    if key not in _DW:
        from vibevoice_rocm_amd.weights import DeviceWeights
        dt, quant, kw, frag = SETS[wset]
        dw = DeviceWeights(cfg_of(geom), sd_of(geom), device, wdtype=dt, streaming_state=False, quant=quant, **kw)
        if frag:
            dw.ensure_frag()
        owned = [t for t in dw._keep if isinstance(t, torch.Tensor)] + list(dw._frag_state["tensors"])
        _DW[key] = (dw, [(t, t.clone()) for t in owned])
    return _DW[key]


def _params_unchanged(snap):
    return all(torch.equal(t.view(torch.uint8), c.view(torch.uint8)) for t, c in snap)


class DevCache:
    """a vv_kv on the device holding the given fp64 cache exactly (bf16 with vt, or fp32 without)"""

    def __init__(self, cfg, k64, v64, dtype):
        L, _ = _lib()
        self.cfg, self.dtype = cfg, dtype
        self.k, self.v = k64.to(dtype).cuda(), v64.to(dtype).cuda()
        self.vt = vt_tiles(self.v) if dtype == BF16 else None
        layers, rows, kvh, s_max, d = k64.shape
        self.kv = L.KV(self.k.data_ptr(), self.v.data_ptr(), L.VV_BF16 if dtype == BF16 else L.VV_F32, layers, rows, kvh, s_max, d,
                       None if self.vt is None else self.vt.data_ptr())

    def bits(self):
        return _bits(self.k.cpu()).clone(), _bits(self.v.cpu()).clone()

    def values(self):
        """the cache's contents as the fp64 cache run_llm starts from"""
        c = new_cache(self.cfg, 1, 1, self.dtype)
        c["k"], c["v"] = self.k.cpu().double(), self.v.cpu().double()
        return c


class DevCache8:
    """an fp8 vv_kv filled on the device from a bf16 DevCache by vv_kv_quantize: row 0 with VV_KVQ_DERIVE_SCALES, the other rows under its scales"""

    def __init__(self, cfg, src, lens):
        L, l = _lib()
        self.cfg, self.lens = cfg, list(lens)
        self.k = torch.full(src.k.shape, FP8_SENTINEL, dtype=torch.uint8, device="cuda")
        self.v = self.k.clone()
        self.vt = vt_tiles(self.v)
        self.kscale = torch.zeros(cfg.layers, cfg.kv_heads, device="cuda")
        self.vscale = torch.zeros_like(self.kscale)
        layers, rows, kvh, s_max, d = src.k.shape
        self.kv = L.KV(self.k.data_ptr(), self.v.data_ptr(), L.VV_FP8, layers, rows, kvh, s_max, d, self.vt.data_ptr(), self.kscale.data_ptr(), self.vscale.data_ptr())
        for r, n in enumerate(lens):
            L.check(l.vv_kv_quantize(C.byref(src.kv), C.byref(self.kv), r, r, n, L.KVQ_DERIVE_SCALES if r == 0 else 0, None), "vv_kv_quantize")
        torch.cuda.synchronize()

    def bits(self):
        return self.k.cpu().clone(), self.v.cpu().clone()

    def values(self):
        ks, vs = self.kscale.cpu(), self.vscale.cpu()
        c = new_cache(self.cfg, 1, 1, BF16)
        c["k"], c["v"] = fp8_values(self.k.cpu(), ks), fp8_values(self.v.cpu(), vs)
        c["rnd"] = lambda t, l, which: (fp8_codes(t, (ks if which == "k" else vs)[l][:, None]).view(F8).float() * (ks if which == "k" else vs)[l][:, None]).double()
        c["dtype"] = F8
        return c


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _nan(*shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device="cuda").view(F32)


def _prof(fn):
    """run fn under the vv_linear profiler: {(m, wdt)} of the launches it recorded"""
    L, l = _lib()
    L.check(l.vv_prof_begin(4096), "vv_prof_begin")
    try:
        fn()
    finally:
        ents = (L.ProfEntry * 256)()
        cnt = C.c_int(0)
        L.check(l.vv_prof_end(ents, 256, C.byref(cnt)), "vv_prof_end")
    return {(ents[i].m, ents[i].wdt) for i in range(cnt.value)}


def expected_forms(wset, R, decode):
    """(weight types the profiler may show for the call, must it show any): the table of the module docstring"""
    dt, quant, kw, frag = SETS[wset]
    if wset == "fp32":
        return {0}, True
    if R <= 2:
        return {WQ_CODE[quant] if quant else 1}, True
    if decode and R <= 8:
        return ({FRAG_CODE[quant]}, True) if wset.endswith("_row_batch") else ({1}, False)      # other sets' rows launches are not recorded
    if decode and R <= 16 and wset == "bf16_frag":
        return {1}, False
    if wset.endswith("_lean") and not decode:
        return {WQ_CODE[quant]}, True
    return {1}, True


def run_call(geom, wset, cache, call, x, prof=False):
    """one vv_llm_forward / vv_llm_prefill_packed call on the device with every guard of the module docstring; returns the output rows (or the
    pre-norm rows at the start of the workspace when out == NULL) on the CPU"""
    L, l = _lib()
    dw, snap = device_weights(geom, wset)
    m, cfg = dw.llm, dw.cfg
    R, H = call["R"], cfg.hidden
    ldx = x.shape[1]
    xbuf = _nan(R, ldx)
    xbuf[:, :H] = x[:, :H].cuda()
    x_before = xbuf.clone()
    lens = torch.tensor(call["lens"], dtype=torch.int32, device="cuda")
    crows = None if call["crows"] is None else torch.tensor(call["crows"], dtype=torch.int32, device="cuda")
    sel = call.get("sel")
    n_out = len(sel) if sel is not None else R
    ldo = H + 8
    out = None if call.get("out_null") else _nan(n_out + 2, ldo)
    nbytes = l.vv_llm_ws_bytes(C.byref(m), R)
    assert nbytes > 0
    guard = -(-nbytes // 256) * 256                         # >= the whole workspace, so >= its largest carve
    wsbuf = torch.full((2 * guard + nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    assert wsbuf.data_ptr() % 256 == 0
    ws = wsbuf.data_ptr() + guard
    if call.get("packed"):
        selt = torch.tensor(sel, dtype=torch.int32, device="cuda")
        assert l.vv_llm_prefill_packed_ws_bytes(C.byref(m), R) == nbytes
        fn = lambda: L.check(l.vv_llm_prefill_packed(C.byref(m), C.byref(cache.kv), xbuf.data_ptr(), ldx, R, lens.data_ptr(), crows.data_ptr(), selt.data_ptr(),
                                                     n_out, out[1].data_ptr(), ldo, ws, None), "vv_llm_prefill_packed")
    else:
        fn = lambda: L.check(l.vv_llm_forward(C.byref(m), C.byref(cache.kv), xbuf.data_ptr(), ldx, R, lens.data_ptr(), None if crows is None else crows.data_ptr(),
                                              None if out is None else out[1].data_ptr(), ldo if out is not None else 0, ws, None), "vv_llm_forward")
    seen = _prof(fn) if prof else fn()
    torch.cuda.synchronize()
    if prof:
        allowed, must = expected_forms(wset, R, call["crows"] is None)
        assert {w for _, w in seen} <= allowed and (seen or not must), f"vv_linear launches (m, weight type) {sorted(seen)}: the table says {sorted(allowed)}"
    assert bool((wsbuf[:guard] == 0xFF).all()) and bool((wsbuf[guard + nbytes:] == 0xFF).all()), f"a guard of the {nbytes}-byte workspace was written"
    assert torch.equal(_bits(xbuf), _bits(x_before)) and lens.cpu().tolist() == list(call["lens"]) and (crows is None or crows.cpu().tolist() == list(call["crows"])), "an input changed"
    assert _params_unchanged(snap), "a parameter changed"
    if out is None:
        return wsbuf[guard: guard + 4 * R * H].view(F32).view(R, H).cpu()
    o = out.cpu()
    ob = _bits(o)
    assert bool((ob[0] == SENT32).all()) and bool((ob[-1] == SENT32).all()), "a guard row of out was written"
    assert bool((ob[1:-1, H:] == SENT32).all()), "the pitch gap of out was written"
    return o[1:-1, :H]


def run_calls(name, geom, wset, cache, calls, record, first=0, state_class=None):
    """the calls on one device cache.  Per call: the reference (run_llm, fp64) starts from the cache AS THE DEVICE HOLDS IT before the call, so a
    call is judged for what it does and not for what its predecessors' roundings left; the figures against it; the slots no row owns; vt.
    Returns per call (out, k bits, v bits) for the repeat check."""
    W = ref_weights(geom, wset)
    cfg = W["cfg"]
    runs = []
    for i, call in enumerate(calls, first):
        kb, vb = cache.bits()
        ref = cache.values()
        x = case_x(name, i, call["R"], cfg.hidden, call.get("ldx_pad", 0))
        want = run_llm(W, x.double(), call["lens"], call["crows"], ref, sel=call.get("sel"), final_norm=not call.get("out_null"))
        got = run_call(geom, wset, cache, call, x, prof=record and i == 0)
        ka, va = cache.bits()
        runs.append((got, ka, va))
        decode = call["crows"] is None
        klass = klass_of(geom, wset, call["R"], decode)[0]
        slots = touched_slots(cfg, call["lens"], range(call["R"]) if decode else call["crows"])
        # every slot no row of the call owns keeps its bits
        mask = torch.ones(ka.shape[1], ka.shape[3], dtype=torch.bool)
        for c, n in slots:
            mask[c, n] = False
        for a, b, what in ((ka, kb, "K"), (va, vb, "V")):
            assert torch.equal(a.permute(1, 3, 0, 2, 4)[mask], b.permute(1, 3, 0, 2, 4)[mask]), f"{name} call {i}: a {what} slot no row owns changed"
        if cache.vt is not None:
            assert torch.equal(_bits(cache.vt), _bits(vt_tiles(cache.v))), f"{name} call {i}: vt != vt_tiles(v)"
        after = cache.values()
        g, row, el = figures(got, want)
        st = state_figure(after["k"], after["v"], ref["k"], ref["v"], slots)
        skey = "state " + (state_class or klass)
        if record:
            rel_rms(got.double().numpy(), want.numpy(), f"{name} call {i} ({klass}): out vs fp64")
            print(f"PARITY llm {klass:<5} {name:<28} call {i} R={call['R']:<4} global {g:.3e} row {row:.3e} element {el:.3e} state {st:.3e} [{skey}]")
        bar, sbar = BAR[klass], BAR[skey]
        assert g < bar and row < bar, f"{name} call {i} ({klass}): global {g:.3e} / worst row {row:.3e} >= {bar:.1e}"
        assert el < ELEM * bar, f"{name} call {i} ({klass}): worst element {el:.3e} >= {ELEM * bar:.1e}"
        assert st < sbar, f"{name} call {i} ({skey}): worst touched K / V slot {st:.3e} >= {sbar:.1e}"
    return runs


def run_case(name, record):
    """all calls of a case on a fresh device cache"""
    case = CASES[name]
    c0 = initial_cache(name)
    cache = DevCache(cfg_of(case["geom"]), c0["k"], c0["v"], c0["dtype"])
    return run_calls(name, case["geom"], case["wset"], cache, case["calls"], record)


def _same_bits(name, a, b, calls, geom, wset):
    for i, ((oa, ka, va), (ob, kb, vb), call) in enumerate(zip(a, b, calls)):
        if any(klass_of(geom, wset, c["R"], c["crows"] is None)[0] == "rows" for c in calls[: i + 1]):
            continue          # split-K slices added with fp32 atomics (gemv_rows_atomic): both runs were held to the bar, and so is what follows on the same cache
        assert torch.equal(_bits(oa), _bits(ob)) and torch.equal(ka, kb) and torch.equal(va, vb), f"{name} call {i}: two runs differ"


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_loop_vs_fp64(name):
    _need_gpu()
    L, l = _lib()
    case = CASES[name]
    packed = any(c.get("packed") for c in case["calls"])
    if packed:
        L.check(l.vv_tune(b"gemm_packed_rows", 64), "vv_tune")
    try:
        a = run_case(name, True)
        b = run_case(name, False)
    finally:
        if packed:
            L.check(l.vv_tune(b"gemm_packed_rows", -1), "vv_tune")
    _same_bits(name, a, b, case["calls"], case["geom"], case["wset"])


KV8_S_MAX = 1088            # > 1024: att_split = 3 and the tickets are memset, on the fp8 cache too
KV8_PROMPTS = (40, 33)      # prompt rows of cache rows 0 and 1: the second ends inside a 32-key tile, one key past it


@gpu
def test_decode_on_an_fp8_cache_vs_fp64():
    """kv8_r2_bf16: two prompts through the loop into a bf16 cache, vv_kv_quantize into an fp8 cache (asserted equal, code for code, to
    quantize_cache of the bf16 cache the device holds), then two decode steps of R = 2 on it - the loop's decode branch with kv->kvdt == VV_FP8.
    The reference's cache holds code * scale and appends its new k / v as saturating e4m3 codes under the head's scale."""
    _need_gpu()
    name, geom, wset = "kv8_r2_bf16", "A", "bf16"
    cfg = cfg_of(geom)
    prompts = [dict(R=n, lens=list(range(n)), crows=[r] * n) for r, n in enumerate(KV8_PROMPTS)]
    steps = [dict(R=2, lens=[n + i for n in KV8_PROMPTS], crows=None) for i in range(2)]
    both = []
    for record in (True, False):
        c0 = new_cache(cfg, 2, KV8_S_MAX, BF16)
        stage = DevCache(cfg, c0["k"], c0["v"], BF16)
        runs = run_calls(name, geom, wset, stage, prompts, record)
        cache = DevCache8(cfg, stage, KV8_PROMPTS)
        staged = stage.values()
        kq, vq, ks, vs = quantize_cache(staged, KV8_PROMPTS)
        assert torch.equal(cache.kscale.cpu(), ks) and torch.equal(cache.vscale.cpu(), vs), "the derived scales differ from the rule's"
        assert torch.equal(cache.k.cpu(), kq) and torch.equal(cache.v.cpu(), vq), "the fp8 cache is not the quantised bf16 cache"
        assert torch.equal(cache.vt, vt_tiles(cache.v)), "vt != vt_tiles(v) after vv_kv_quantize"
        runs += run_calls(name, geom, wset, cache, steps, record, first=2, state_class="kv8")
        both.append(runs)
    _same_bits(name, both[0], both[1], prompts + steps, geom, wset)


# ---------------------------------------------------------------------------------------------------------------
# refusals: decided on the host before the first launch, so they are asserted with or without a GPU
# ---------------------------------------------------------------------------------------------------------------
class _Args:
    """arguments of a refused call: real device buffers where there is a GPU, stand-in addresses where there is none (a refusal follows no
    data pointer; without the refusal a box with no GPU answers VV_E_HIP from the first launch)"""

    def __init__(self, geom, wset, R, rows, s_max=64):
        L, l = _lib()
        self.dev = "cuda" if torch.cuda.is_available() else "cpu"
        self.dw, _ = device_weights(geom, wset, self.dev)
        cfg = self.dw.cfg
        self.keep = []
        alloc_rows = max(rows, R) + 1                          # the allocation is larger than the cache the descriptor declares
        n_kv = cfg.layers * alloc_rows * cfg.kv_heads * s_max * cfg.head_dim
        self.k, self.v, self.vt = (self.buf(2 * n_kv) for _ in range(3))
        self.kv = L.KV(self.k, self.v, L.VV_BF16, cfg.layers, rows, cfg.kv_heads, s_max, cfg.head_dim, self.vt)
        self.x, self.out = self.buf(4 * R * cfg.hidden), self.buf(4 * R * cfg.hidden)
        self.lens, self.crows = self.buf(4 * R, ints=list(range(R))), self.buf(4 * R, ints=[0] * R)       # with cache_rows: a prompt on cache row 0
        self.ws = self.buf(max(l.vv_llm_ws_bytes(C.byref(self.dw.llm), R), 256))
        self.R, self.H = R, cfg.hidden

    def buf(self, nbytes, ints=None):
        if self.dev == "cpu":
            self.keep.append(None)
            return 0x10000000 + 0x1000000 * len(self.keep)
        t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda") if ints is None else torch.tensor(ints, dtype=torch.int32, device="cuda")
        self.keep.append(t)
        return t.data_ptr()

    def forward(self, crows):
        _, l = _lib()
        return l.vv_llm_forward(C.byref(self.dw.llm), C.byref(self.kv), self.x, self.H, self.R, self.lens, self.crows if crows else None, self.out, self.H, self.ws, None)


def _refused(rc, code, *words):
    _, l = _lib()
    msg = l.vv_last_error().decode()
    assert rc == code, f"returned {rc} ({msg}), expected {code}"
    for w in words:
        assert w in msg, msg


@pytest.mark.parametrize("wset", ["mxfp4_lean", "mxfp6_lean"])
@pytest.mark.parametrize("R", [3, 8, 9, 16])
def test_lean_decode_of_3_to_16_rows_is_refused(wset, R):
    """no bf16 matrix and no fragment copies: a 3..8-row decode pass has nothing to run on, a 9..16-row pass never has"""
    a = _Args("A", wset, R, rows=16)
    _refused(a.forward(crows=False), VV_E_UNSUPPORTED, "lean", "decode pass")


def test_packed_prefill_on_an_fp8_cache_is_refused():
    L, l = _lib()
    a = _Args("A", "bf16", 64, rows=2, s_max=96)
    a.kv.kvdt = L.VV_FP8
    sel = a.buf(16, ints=[0])
    rc = l.vv_llm_prefill_packed(C.byref(a.dw.llm), C.byref(a.kv), a.x, a.H, 64, a.lens, a.crows, sel, 1, a.out, a.H, a.ws, None)
    _refused(rc, VV_E_UNSUPPORTED, "fp8 KV cache")


@pytest.mark.parametrize("field", ["layers", "kv_heads", "head_dim"])
def test_a_cache_of_another_shape_is_refused(field):
    a = _Args("A", "bf16", 2, rows=2)
    setattr(a.kv, field, getattr(a.kv, field) // 2)           # a smaller cache than allocated: nothing is out of bounds even unrefused
    _refused(a.forward(crows=False), VV_E_ARG, "kv cache shape")


@pytest.mark.parametrize("R,rows", [(3, 2), (2, 1), (17, 16), (64, 2)])
def test_more_rows_than_cache_rows_without_cache_rows_is_refused(R, rows):
    """cache_rows == NULL means row r owns cache row r: R > kv->rows would store rows >= kv->rows outside the cache.  vv_llm_forward,
    vv_rope_store and vv_attn each answer VV_E_ARG before the first launch (without the check, a box with no GPU answers VV_E_HIP)."""
    L, l = _lib()
    a = _Args("A", "bf16", R, rows=rows)
    _refused(a.forward(crows=False), VV_E_ARG, "cache rows")
    cfg = a.dw.cfg
    qkvd = (cfg.heads + 2 * cfg.kv_heads) * cfg.head_dim
    qkv, rope, att = a.buf(4 * R * qkvd), a.buf(4 * R * cfg.head_dim), a.buf(4 * R * cfg.heads * cfg.head_dim)
    _refused(l.vv_rope_store(qkv, qkvd, R, cfg.heads, C.byref(a.kv), 0, rope, a.lens, None, None), VV_E_ARG, "vv_rope_store", "cache rows")
    _refused(l.vv_attn(qkv, qkvd, R, cfg.heads, C.byref(a.kv), 0, a.lens, None, att, cfg.heads * cfg.head_dim, None), VV_E_ARG, "vv_attn", "cache rows")
    if torch.cuda.is_available():                              # ... and with cache_rows the same call is taken (a prompt of R rows on cache row 0)
        L.check(a.forward(crows=True), "vv_llm_forward with cache_rows")
        torch.cuda.synchronize()
