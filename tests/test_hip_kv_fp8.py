"""The optional fp8 (e4m3) KV cache of the decode steps (include/vv_hip.h: vv_kv.kvdt == VV_FP8, vv_kv_quantize, vv_attn_decode) on the GPU.

Kernel level (head_dim 128, 2 KV heads, 12 / 14 q heads = groups of 6 and 7, 2 layers with layer 1 under test, s_max 1024, two rows with different
positions): vv_kv_quantize byte for byte against torch; the fp8 instantiation of the grouped-query decode kernel BIT-IDENTICAL to the bf16
instantiation on the dequantised cache (an e4m3 value times a power of two is exact in bf16, and everything behind the widening is the same
instruction sequence), unsplit and with the keys split over workgroups; the append; the refusals.
Engine level (`mid` synthetic config): generate() with kv_cache_dtype="fp8" - graph == eager, repeatable, the cache after prefill, the waveform
deviation against the project's accepted lossy mode, and a batch of two on the lanes."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import rel_rms, vt_tiles

pytestmark = pytest.mark.gpu

D, LAYERS, ROWS, KVH, S_MAX, LAYER = 128, 2, 2, 2, 1024, 1
F8 = torch.float8_e4m3fn


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class _Tok:
    def __init__(self, v):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = v - 4, v - 3, v - 2, v - 1
        self.bos_token_id, self.pad_id = None, 0


def _lib():
    from vibevoice_rocm_amd import _lib as L
    return L, L.load()


def _kv(L, k, v, vt, kvdt, s_max, scales=None, rows=ROWS):
    kv = L.KV(k.data_ptr(), v.data_ptr(), kvdt, LAYERS, rows, KVH, s_max, D, vt.data_ptr())
    if scales is not None:
        kv.kscale, kv.vscale = scales[0].data_ptr(), scales[1].data_ptr()
    return kv


def _codes(x, scale):
    """e4m3fn codes of x under `scale` (broadcastable), saturating: torch's cast does not saturate, so clamp first"""
    return (x.float() / scale).clamp(-448, 448).to(F8).view(torch.uint8)


def _dequant(codes, scale):
    """bf16 cache holding fp32(code) * scale exactly"""
    y = codes.view(F8).float() * scale
    out = y.to(torch.bfloat16)
    assert torch.equal(out.float(), y), "e4m3 x 2^p is exact in bf16"
    return out


def _scale_rule(absmax):
    a = absmax.double()
    return torch.where(a == 0, torch.ones_like(a), torch.exp2(torch.ceil(torch.log2(a / 224.0)))).float()


# ---------------------------------------------------------------------------------------------------------------
# 1. vv_kv_quantize
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 31, 32, 33, 700])
def test_kv_quantize_vs_torch(n):
    """Row 0 of a bf16 cache (s_max 768: the staging cache is sized to the prompt) into row 0 of an fp8 cache (s_max 1024) deriving the scales,
    then row 1 under the same scales.  Row 1 holds a head whose values exceed 448 x scale: its codes saturate to +-448 (0x7e / 0xfe), never the
    NaN code.  One V head of row 0 is all zero (scale 1).  Slots >= len of k, v and the tile-major vt keep their sentinel byte."""
    _need_gpu()
    L, lib = _lib()
    g = torch.Generator().manual_seed(100 + n)
    s_src = 768
    mag = torch.tensor([[0.3, 40.0], [7.0, 900.0]])[:, None, :, None, None]             # per (layer, kv head): scales well apart
    ks = (torch.randn(LAYERS, ROWS, KVH, s_src, D, generator=g) * mag).to(torch.bfloat16)
    vs = (torch.randn(LAYERS, ROWS, KVH, s_src, D, generator=g) * mag.flip(2)).to(torch.bfloat16)
    vs[0, 0, 1] = 0                                                                       # an all-zero head: scale 1
    ks[1, 1, 0] *= 40                                                                     # row 1 overshoots row 0's scale: saturation
    vs[1, 1, 1, :, ::3] *= -25
    ks[:, 0, :, n:] = 1e30                                                                # slots >= len must not enter the absmax
    vs[:, 0, :, n:] = -1e30
    sent = 0x5A
    kd = torch.full((LAYERS, ROWS, KVH, S_MAX, D), sent, dtype=torch.uint8, device="cuda")
    vd, vtd = kd.clone(), kd.clone().view(LAYERS, ROWS, KVH, S_MAX // 32, D, 32)
    sc = torch.full((2, LAYERS, KVH), -7.0, device="cuda")
    ksd, vsd = ks.cuda(), vs.cuda()
    src = _kv(L, ksd, vsd, vt_tiles(vsd), L.VV_BF16, s_src)
    dst = _kv(L, kd, vd, vtd, L.VV_FP8, S_MAX, sc)
    L.check(lib.vv_kv_quantize(C.byref(src), C.byref(dst), 0, 0, n, L.KVQ_DERIVE_SCALES, None), "vv_kv_quantize row 0")
    L.check(lib.vv_kv_quantize(C.byref(src), C.byref(dst), 1, 1, n, 0, None), "vv_kv_quantize row 1")
    torch.cuda.synchronize()
    want_sc = torch.stack([_scale_rule(ks[:, 0, :, :n].float().abs().amax((-1, -2))), _scale_rule(vs[:, 0, :, :n].float().abs().amax((-1, -2)))])
    assert torch.equal(sc.cpu(), want_sc), (sc.cpu(), want_sc)
    assert float(want_sc[1, 0, 1]) == 1.0
    wk = torch.full((LAYERS, ROWS, KVH, S_MAX, D), sent, dtype=torch.uint8)
    wv = wk.clone()
    wk[:, :, :, :n] = _codes(ks[:, :, :, :n], want_sc[0][:, None, :, None, None])
    wv[:, :, :, :n] = _codes(vs[:, :, :, :n], want_sc[1][:, None, :, None, None])
    assert torch.equal(kd.cpu(), wk), "k codes / untouched slots"
    assert torch.equal(vd.cpu(), wv), "v codes / untouched slots"
    assert torch.equal(vtd.cpu(), vt_tiles(wv)), "vt = tile-major permutation of v, slots >= len untouched"
    got = torch.cat([kd.cpu()[:, :, :, :n].reshape(-1), vd.cpu()[:, :, :, :n].reshape(-1)])
    assert int(((got & 0x7f) == 0x7f).sum()) == 0, "the NaN code is never produced"
    sat_k = kd.cpu()[1, 1, 0, :n]
    assert int(((sat_k & 0x7f) == 0x7e).sum()) > 0, "the overshooting head saturates to +-448"


# ---------------------------------------------------------------------------------------------------------------
# 2. + 3.  the fp8 instantiation against the bf16 instantiation, and the append
# ---------------------------------------------------------------------------------------------------------------
def _random_fp8_cache(g):
    k8 = torch.randint(0, 256, (LAYERS, ROWS, KVH, S_MAX, D), generator=g, dtype=torch.int32).to(torch.uint8)
    v8 = torch.randint(0, 256, (LAYERS, ROWS, KVH, S_MAX, D), generator=g, dtype=torch.int32).to(torch.uint8)
    for t in (k8, v8):
        t[(t & 0x7f) == 0x7f] = 0x3c                       # no NaN codes: NaN == NaN would not compare equal
    sc = torch.exp2(torch.randint(-3, 4, (2, LAYERS, KVH), generator=g).float())
    return k8, v8, sc


def _bc(sc, i):
    return sc[i][:, None, :, None, None]


class _Attn:
    """one vv_attn_decode call on device copies of a cache; mode: 0 = unsplit (the public entry point), n > 0 = keys split n ways"""

    def __init__(self, heads):
        self.L, self.lib = _lib()
        self.heads = heads
        self.ld = (heads + 2 * KVH) * D
        self.inv_freq = (1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float32) / D))).cuda()

    def rope(self, lens_d):
        rope = torch.empty(ROWS, D // 2, 2, device="cuda")
        self.L.check(self.lib.vv_rope_table(lens_d.data_ptr(), self.inv_freq.data_ptr(), ROWS, D, rope.data_ptr(), None), "vv_rope_table")
        return rope

    def run(self, kv, qkv_d, lens_d, rope, mode, gqa_keys=1024):
        L, lib = self.L, self.lib
        out = torch.full((ROWS, self.heads * D), float("nan"), device="cuda")
        lib.vv_tune(b"attn_gqa", 2)                        # 2 = the grouped kernel whatever the context length (1 picks it by context length: at
        lib.vv_tune(b"attn_gqa_keys", gqa_keys)            # s_max 1024 the bf16 side would run the per-head kernel)
        try:
            if mode == 0:
                rc = lib.vv_attn_decode(qkv_d.data_ptr(), self.ld, ROWS, self.heads, C.byref(kv), LAYER, rope.data_ptr(), lens_d.data_ptr(), out.data_ptr(),
                                        self.heads * D, None)
            else:
                cap = max(mode, S_MAX // gqa_keys)
                part = torch.empty(lib.vv_attn_decode_part_floats(ROWS, self.heads, cap), device="cuda")
                tickets = torch.zeros(ROWS * self.heads, dtype=torch.int32, device="cuda")
                rc = lib.vv_attn_decode_split(qkv_d.data_ptr(), self.ld, ROWS, self.heads, C.byref(kv), LAYER, rope.data_ptr(), lens_d.data_ptr(),
                                              out.data_ptr(), self.heads * D, part.data_ptr(), tickets.data_ptr(), mode, cap, None)
            L.check(rc, "vv_attn_decode")
            torch.cuda.synchronize()
            if mode:
                assert int(tickets.abs().sum()) == 0, "tickets are left zero"
        finally:
            lib.vv_tune(b"attn_gqa", 1)
            lib.vv_tune(b"attn_gqa_keys", 1024)
        return out.cpu()


@pytest.fixture(scope="module")
def fp8_cache():
    g = torch.Generator().manual_seed(77)
    k8, v8, sc = _random_fp8_cache(g)
    return k8, v8, sc, _dequant(k8, _bc(sc, 0)), _dequant(v8, _bc(sc, 1))


@pytest.mark.parametrize("heads", [12, 14])
@pytest.mark.parametrize("lens", [(0, 5), (31, 32), (33, 257), (700, 255)])
def test_fp8_decode_attention_bit_identical_to_bf16_kernel(fp8_cache, heads, lens):
    """Random e4m3 codes and random power-of-two scales against a bf16 cache holding the dequantised values, the grouped-query kernel on both
    sides (vv_tune attn_gqa 2: "always"; value 1 chooses by context length and would run the per-head kernel on the bf16 side at this s_max),
    same qkv, same key split: the attention outputs are bit-identical - unsplit, with the keys split 3 ways (per = ceil(pos / 3) rounded up to
    whole 32-key tiles: position 33 fills 2 of the 3 splits, 257 all 3, 5 one, 0 none - rows of one launch with different live split counts)
    and 4 ways through vv_tune attn_gqa_keys 256.  No shape here sums in a different order: both instantiations share every instruction
    behind the widening of the cache fragments.  Slots behind the position hold random codes on both sides."""
    _need_gpu()
    k8, v8, sc, kb, vb = fp8_cache
    A = _Attn(heads)
    L = A.L
    g = torch.Generator().manual_seed(heads * 1000 + sum(lens))
    qkv_d = torch.randn(ROWS, A.ld, generator=g).cuda()
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    rope = A.rope(lens_d)
    for mode, keys in ((0, 1024), (3, 1024), (2, 256)):
        k8d, v8d, scd = k8.cuda(), v8.cuda(), sc.cuda()
        vt8d = vt_tiles(v8d)
        o8 = A.run(_kv(L, k8d, v8d, vt8d, L.VV_FP8, S_MAX, scd), qkv_d, lens_d, rope, mode, keys)
        kbd, vbd = kb.cuda(), vb.cuda()
        vtbd = vt_tiles(vbd)
        o16 = A.run(_kv(L, kbd, vbd, vtbd, L.VV_BF16, S_MAX), qkv_d, lens_d, rope, mode, keys)
        assert bool(torch.isfinite(o8).all())
        assert torch.equal(o8, o16), f"heads {heads} lens {lens} mode {mode} keys/split {keys}: max |diff| {float((o8 - o16).abs().max()):.3e}"


@pytest.mark.parametrize("heads", [12, 14])
def test_fp8_decode_append_and_second_step(fp8_cache, heads):
    """After a step, slot lens[r] of k, v and vt of row r holds the saturated codes of RoPE(k_new) and v_new under the head's scale and every
    other byte of the three arrays is unchanged; a second step at lens + 1 reads the appended slot: its output equals the bf16 kernel's on
    the cache dequantised after step 1.  v is copied, so its codes are exact.  RoPE(k_new) is recomputed in fp64 from the same rope_table; the
    kernel forms it in fp32 (one fused multiply-add: relative error <= 2^-23 of the larger product, far below 1e-5), so a code may differ
    from the fp64 one only where the value lies within 1e-5 (relative) of a rounding boundary: the code must equal the fp64 code of
    x (1 - 1e-5) or of x (1 + 1e-5).  One K head and one V head of the new token are scaled by 4000, so that many of their elements overshoot 448 x scale (scale <= 8)."""
    _need_gpu()
    k8, v8, sc, _, _ = fp8_cache
    A = _Attn(heads)
    L = A.L
    lens = (700, 255)
    g = torch.Generator().manual_seed(heads)
    qkv = torch.randn(ROWS, A.ld, generator=g)
    qkv[0, heads * D: (heads + 1) * D] *= 4000.0                              # row 0, KV head 0: k overshoots
    qkv[1, (heads + KVH + 1) * D: (heads + KVH + 2) * D] *= 4000.0           # row 1, KV head 1: v overshoots
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    rope = A.rope(lens_d)
    k8d, v8d, scd = k8.cuda(), v8.cuda(), sc.cuda()
    vt8d = vt_tiles(v8d)
    kv8 = _kv(L, k8d, v8d, vt8d, L.VV_FP8, S_MAX, scd)
    A.run(kv8, qkv.cuda(), lens_d, rope, 0)
    k1, v1, vt1 = k8d.cpu(), v8d.cpu(), vt8d.cpu()
    wk, wv = k8.clone(), v8.clone()
    tab = rope.cpu().double()
    for r in range(ROWS):
        kn = qkv[r, heads * D: (heads + KVH) * D].view(KVH, D).double()
        c, s_ = tab[r, :, 0], tab[r, :, 1]
        x1, x2 = kn[:, : D // 2], kn[:, D // 2:]
        kr = torch.cat([x1 * c - x2 * s_, x2 * c + x1 * s_], -1)
        ksc = sc[0, LAYER].double()[:, None]
        lo, hi = _codes(kr * (1 - 1e-5), ksc), _codes(kr * (1 + 1e-5), ksc)
        got = k1[LAYER, r, :, lens[r]]
        assert bool(((got == lo) | (got == hi)).all()), f"row {r}: appended k codes"
        assert float((got == _codes(kr, ksc)).float().mean()) > 0.98
        wk[LAYER, r, :, lens[r]] = got
        wv[LAYER, r, :, lens[r]] = _codes(qkv[r, (heads + KVH) * D:].view(KVH, D), sc[1, LAYER][:, None])
    # saturation: wherever the new value exceeds 448 x scale the code is +-448 (0x7e / 0xfe); both overshooting heads have such elements
    v_over = (qkv[1, (heads + KVH + 1) * D: (heads + KVH + 2) * D].double().abs() > 448.0 * float(sc[1, LAYER, 1]))
    k0 = qkv[0, heads * D: (heads + 1) * D].double()
    k_over = (torch.cat([k0[: D // 2] * tab[0, :, 0] - k0[D // 2:] * tab[0, :, 1], k0[D // 2:] * tab[0, :, 0] + k0[: D // 2] * tab[0, :, 1]]).abs()
              > 448.0 * float(sc[0, LAYER, 0]) * (1 + 1e-5))
    assert int(v_over.sum()) > 0 and int(k_over.sum()) > 0
    assert bool(((v1[LAYER, 1, 1, lens[1]] & 0x7f) == 0x7e)[v_over].all()) and bool(((k1[LAYER, 0, 0, lens[0]] & 0x7f) == 0x7e)[k_over].all()), "saturated, not NaN"
    assert int(((k1 & 0x7f) == 0x7f).sum()) == 0 and int(((v1 & 0x7f) == 0x7f).sum()) == 0
    assert torch.equal(k1, wk), "k: the appended slot and nothing else"
    assert torch.equal(v1, wv), "v: the appended slot holds the codes of v_new, nothing else changed"
    assert torch.equal(vt1, vt_tiles(wv)), "vt stays the tile-major permutation of v"
    # second step: the appended slot is read
    lens2 = torch.tensor([n + 1 for n in lens], dtype=torch.int32).cuda()
    rope2 = A.rope(lens2)
    qkv2 = torch.randn(ROWS, A.ld, generator=g).cuda()
    o8 = A.run(kv8, qkv2, lens2, rope2, 0)
    kbd, vbd = _dequant(k1, _bc(sc, 0)).cuda(), _dequant(v1, _bc(sc, 1)).cuda()
    vtbd = vt_tiles(vbd)
    o16 = A.run(_kv(L, kbd, vbd, vtbd, L.VV_BF16, S_MAX), qkv2, lens2, rope2, 0)
    assert torch.equal(o8, o16), f"second step: max |diff| {float((o8 - o16).abs().max()):.3e}"
    # ... and it matters: the same step without the appended slot gives another answer
    o_prev = A.run(_kv(L, k8.cuda(), v8.cuda(), vt_tiles(v8.cuda()), L.VV_FP8, S_MAX, scd), qkv2, lens2, rope2, 0)
    assert not torch.equal(o8, o_prev)


# ---------------------------------------------------------------------------------------------------------------
# 4. refusals (status codes only: nothing is launched)
# ---------------------------------------------------------------------------------------------------------------
def test_fp8_cache_is_refused_outside_the_grouped_decode_kernel():
    _need_gpu()
    L, lib = _lib()
    heads = 12
    k = torch.zeros(LAYERS, ROWS, KVH, 64, D, dtype=torch.uint8, device="cuda")
    v, vt = k.clone(), k.clone()
    sc = torch.ones(2, LAYERS, KVH, device="cuda")
    kv = _kv(L, k, v, vt, L.VV_FP8, 64, sc)
    ld = (heads + 2 * KVH) * D
    qkv = torch.zeros(ROWS, ld, device="cuda")
    lens = torch.zeros(ROWS, dtype=torch.int32, device="cuda")
    rope = torch.zeros(ROWS, D // 2, 2, device="cuda")
    out = torch.zeros(ROWS, heads * D, device="cuda")
    UNSUPPORTED = -3
    assert lib.vv_rope_store(qkv.data_ptr(), ld, ROWS, heads, C.byref(kv), LAYER, rope.data_ptr(), lens.data_ptr(), None, None) == UNSUPPORTED
    assert b"fp8" in lib.vv_last_error()
    assert lib.vv_attn(qkv.data_ptr(), ld, ROWS, heads, C.byref(kv), LAYER, lens.data_ptr(), None, out.data_ptr(), heads * D, None) == UNSUPPORTED
    assert b"fp8" in lib.vv_last_error()
    lib.vv_tune(b"attn_gqa", 0)                            # the per-head kernel
    try:
        rc = lib.vv_attn_decode(qkv.data_ptr(), ld, ROWS, heads, C.byref(kv), LAYER, rope.data_ptr(), lens.data_ptr(), out.data_ptr(), heads * D, None)
    finally:
        lib.vv_tune(b"attn_gqa", 1)
    assert rc == UNSUPPORTED and b"per-head" in lib.vv_last_error()
    kv.kscale = None                                       # an fp8 cache without scales
    assert lib.vv_attn_decode(qkv.data_ptr(), ld, ROWS, heads, C.byref(kv), LAYER, rope.data_ptr(), lens.data_ptr(), out.data_ptr(), heads * D, None) == UNSUPPORTED
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0 and int(k.sum()) == 0


# ---------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    cfg = VVConfig.preset("mid")
    sd = synth_state_dict_torch(cfg, 4242, device="cuda:0", dtype=torch.bfloat16)
    models = {}

    def get(name):
        if name not in models:
            kw = dict(bf16={}, kv8=dict(kv_cache_dtype="fp8"), w8=dict(weight_quant="fp8"))[name]
            models[name] = M(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, **kw)
            models[name].set_ddpm_inference_steps(10)
        return models[name]
    yield cfg, get
    for m in models.values():
        m.release_lanes()
        m.engine.close()


def _call(cfg, seed=9):
    """forced tokens, injected noise, one 2-frame voice prompt, one turn switch (speech_end, speech_start: the negative branch is reset), 6 frames"""
    V = cfg.vocab
    ST, SE, SD, EOS = V - 4, V - 3, V - 2, V - 1
    g = torch.Generator().manual_seed(seed)
    ids = torch.cat([torch.randint(0, 1000, (39,), generator=g), torch.tensor([ST])])
    forced = [SD, SD, SD, SE, ST, SD, SD, SD, SE, EOS]
    sp_mask = torch.zeros(40, dtype=torch.bool)
    sp_mask[7:9] = True
    return dict(input_ids=ids[None], speech_tensors=0.1 * torch.randn(1, 2 * cfg.hop - 321, generator=g), speech_masks=torch.ones(1, 2, dtype=torch.bool),
                speech_input_mask=sp_mask[None], tokenizer=_Tok(V), cfg_scale=2.0, forced_tokens=forced, noise=torch.randn(6, cfg.latent, generator=g),
                speech_noise=(torch.randn(1, generator=g), torch.randn(1, 2, cfg.ac_dim, generator=g))), forced


def test_generate_fp8_kv_graph_equals_eager_and_repeats(mid):
    cfg, get = mid
    m = get("kv8")
    assert m.engine.kv_fp8
    kw, forced = _call(cfg)
    a = m.generate(**kw)
    assert a.sequences[0, 40:].tolist() == forced
    wa = a.speech_outputs[0]
    assert tuple(wa.shape) == (1, 6 * cfg.hop) and bool(torch.isfinite(wa).all()) and float(wa.abs().max()) > 0
    eng = m.engine
    assert eng.kv.kvdt == 2 and eng._kv_t[0].dtype == torch.uint8 and eng._kv_vt.dtype == torch.uint8 and eng.kv.kscale and eng.kv.vscale
    b = m.generate(**kw)
    assert torch.equal(wa, b.speech_outputs[0]), "two calls must be bit-identical"
    m.engine.use_graphs = False
    try:
        c = m.generate(**kw)
    finally:
        m.engine.use_graphs = True
    assert torch.equal(wa, c.speech_outputs[0]), "hipGraph replay must equal eager launches"


def test_fp8_cache_after_prefill_is_the_quantised_bf16_cache(mid):
    """The byte caches and scales an fp8-KV engine holds after the prompt prefill equal vv_kv_quantize of a bf16-KV engine's cache after the same
    prefill (the staging cache changes the strides, not the values)."""
    cfg, get = mid
    L, lib = _lib()
    e8, e16 = get("kv8").engine, get("bf16").engine
    ids = torch.randint(0, 1000, (45,), generator=torch.Generator().manual_seed(2))
    n = int(ids.numel())
    valid = [cfg.vocab - 4, cfg.vocab - 3, cfg.vocab - 2, cfg.vocab - 1]
    for e in (e8, e16):
        e.begin_sequence(256, valid)
        e.prefill(e.embed_ids(ids), row=0, pos0=0, neg_embed=e.embed_ids(torch.tensor([cfg.vocab - 4])))
        e.stream.synchronize()
    assert torch.equal(e8.hidden2, e16.hidden2) and e8.lens.tolist() == [n, 0]
    s_max = e8.kv.s_max
    shape = (cfg.layers, 2, cfg.kv_heads, s_max, cfg.head_dim)
    k = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    v = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    vt = torch.zeros((cfg.layers, 2, cfg.kv_heads, s_max // 32, cfg.head_dim, 32), dtype=torch.uint8, device="cuda")
    sc = torch.zeros(2, cfg.layers, cfg.kv_heads, device="cuda")
    dst = L.KV(k.data_ptr(), v.data_ptr(), L.VV_FP8, cfg.layers, 2, cfg.kv_heads, s_max, cfg.head_dim, vt.data_ptr(), sc[0].data_ptr(), sc[1].data_ptr())
    with torch.cuda.stream(e16.stream):
        L.check(lib.vv_kv_quantize(C.byref(e16.kv), C.byref(dst), 0, 0, n, L.KVQ_DERIVE_SCALES, e16.sp), "quantize row 0")
        L.check(lib.vv_kv_quantize(C.byref(e16.kv), C.byref(dst), 1, 1, 1, 0, e16.sp), "quantize row 1")
    e16.stream.synchronize()
    assert torch.equal(e8._kv_scale, sc) and bool((sc > 0).all())
    for r, ln in ((0, n), (1, 1)):
        assert torch.equal(e8._kv_t[0][:, r, :, :ln], k[:, r, :, :ln]) and torch.equal(e8._kv_t[1][:, r, :, :ln], v[:, r, :, :ln])
        for s in range(ln):
            assert torch.equal(e8._kv_vt[:, r, :, s // 32, :, s % 32], vt[:, r, :, s // 32, :, s % 32])
    assert int(k[:, 0, :, :n].ne(0).sum()) > 0


def test_fp8_kv_deviation_against_the_accepted_lossy_mode(mid):
    """Quality yardstick, measured here: waveform relative RMS of the fp8-KV run against the bf16-KV run must not exceed that of
    weight_quant="fp8" (bf16 KV), the project's accepted lossy mode, against the same bf16 run - margin x1: both are one e4m3 rounding of one
    operand class."""
    cfg, get = mid
    kw, _ = _call(cfg)
    ref = get("bf16").generate(**kw).speech_outputs[0][0].float().cpu().numpy()
    kv8 = get("kv8").generate(**kw).speech_outputs[0][0].float().cpu().numpy()
    w8 = get("w8").generate(**kw).speech_outputs[0][0].float().cpu().numpy()
    e_kv = rel_rms(kv8, ref, "generate() mid bf16: kv_cache_dtype='fp8' vs bf16 KV, waveform")
    e_w8 = rel_rms(w8, ref, "generate() mid bf16: weight_quant='fp8' (bf16 KV) vs plain bf16, waveform (the yardstick)")
    print(f"fp8 KV deviation {e_kv:.4e}, weight-only fp8 deviation {e_w8:.4e}")
    assert e_kv <= e_w8, f"fp8 KV waveform rel RMS {e_kv:.4e} exceeds the weight-only fp8 yardstick {e_w8:.4e} (margin x1)"


def test_fp8_kv_batch_of_two_runs_on_the_lanes_and_equals_single_runs(mid):
    cfg, get = mid
    m = get("kv8")
    tok = _Tok(cfg.vocab)
    Dn, E, S, EOS = tok.speech_diffusion_id, tok.speech_end_id, tok.speech_start_id, tok.eos_token_id
    g = torch.Generator().manual_seed(31)
    ids = torch.stack([torch.cat([torch.randint(0, 1000, (29,), generator=g), torch.tensor([S])]) for _ in range(2)])
    forced = [[Dn] * 3 + [E, S] + [Dn] * 2 + [E, EOS], [Dn] * 4 + [E, EOS]]
    noise = torch.randn(2, 6, cfg.latent, generator=g)
    both = m.generate(input_ids=ids, attention_mask=torch.ones_like(ids), tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    assert not m._rowbatch, "an fp8-KV batch runs on the lanes (RowBatch needs a bf16 cache)"
    assert len(m._lanes) == 2 and all(e.kv_fp8 for e in m._lanes)
    for b in range(2):
        one = m.generate(input_ids=ids[b][None], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[b], noise=noise[b])
        assert both.sequences[b, 30: 30 + len(forced[b])].tolist() == forced[b]
        assert torch.equal(both.speech_outputs[b].reshape(-1), one.speech_outputs[0].reshape(-1)), f"dialogue {b}: the lane equals the single run"
    from vibevoice_rocm_amd import _lib as Lm
    from vibevoice_rocm_amd.rowbatch import RowBatch
    with pytest.raises(Lm.VVError, match="fp8"):
        RowBatch(m._lanes[:2], stream=m.engine.stream)
