"""Every decode-attention path against one fp64 reference - all `-m gpu`, all through the C ABI, no engine and no model weights.

  A  split-key per-head kernel (attn_decode_kernel<8>, vv_tune attn_gqa 0), nsplit 2 / 3 / 7 / 16, rows with different numbers of empty splits
  B  split-key grouped matrix-core kernel (attn_decode_gqa_kernel, attn_gqa 2) at every fold width and its edges (2 .. 64 launched splits), G = 1, 6, 7, 8
  C  the default rule (attn_gqa 1) on both sides of kv_heads * s_max >= 12288 with the split count vv_llm_forward computes
  D  the LLM step's workspace reuse: one partials buffer and one ticket array for two layers, eager and as a replayed hipGraph
  E  the appended k / v / v^T slots and every other byte of the cache (checked inside A - C)
  F  the generic kernel (attn_fused_kernel) on fp32 / head_dim 64 caches, driven past one, two and three strides of its double-buffered loop
  G  vv_rope_table against fp64 cos / sin of the fp32 angle at positions up to 100 000

The reference (`ref_decode_fp64`) is plain torch fp64 on the cache contents as the device received them; it knows nothing of tiles or splits.
Bars: 2e-4 global rel RMS per call (the project's bar for these kernels unsplit; the split route adds one fp32 fold) and 1e-3 for the worst
(row, head) of a call - ten times below the 1e-2 that the planted-edge check shows a single dropped or doubled boundary key to cost.

Measured on the MI355X, largest value over the group's calls, global / worst (row, head) rel RMS against fp64:
  per-head kernel, split (A, and the same inputs of B, C)    1.9e-7 / 5.0e-7     peaky data 1.9e-7 / 1.2e-6
  grouped kernel, split (B, and the same inputs of A, C)     3.3e-6 / 7.8e-6     peaky data 3.4e-6 / 2.4e-5
  default rule (C)                                           3.3e-6 / 5.1e-6     (s_max 6144; 1.9e-7 / 3.7e-7 at s_max 6112)
  workspace reuse, eager and replayed graph (D)              per-head 1.8e-7 / 2.5e-7, grouped 3.2e-6 / 6.7e-6; replays bit-identical
  generic kernel (F)                                         fp32 d=64 1.9e-7 / 3.0e-7, fp32 d=128 1.8e-7 / 2.6e-7, bf16 d=64 1.9e-7 / 3.3e-7
  appended k (E)                                             bf16 caches 1.9e-3 (one bf16 rounding), fp32 caches 4.5e-8; v, v^T exact
  rope table (G), max abs error                              d=128 6.2e-8 (position 65 535), d=64 5.2e-8
No value is within a factor of two of its bar: the largest, 2.4e-5 for one (row, head) of the grouped kernel on peaky data at 2 splits, is 40 times
below 1e-3.  The grouped kernel's hi + lo bf16 operand split (2^-17 relative) is what sets its level ~ 20 times above the per-head kernel's.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from conftest import rel_rms, vt_tiles

pytestmark = pytest.mark.gpu

GLOBAL_BAR = 2e-4      # rel RMS of a whole call against fp64
HEAD_BAR = 1e-3        # rel RMS of the worst (row, head) of a call against fp64
EDGE_COST = 1e-2       # what one dropped / doubled planted key must cost at least one (row, head) (checked on the CPU)
K_BF16_BAR = 4e-3      # appended rotated key against the unrounded fp64 one: bf16 rounding only (2^-9 / sqrt(3) = 1.1e-3 rel RMS)
K_F32_BAR = 16 * 2.0 ** -24   # fp32 cache: cosf / sinf to a few ulp, two products and one sum in fp32 - 16 half-ulps is a generous ceiling
ROPE_BAR = 4 * 2.0 ** -23     # absolute: cosf / sinf are correct to a few ulp of values in [-1, 1]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


_LIB = []


def _lib():
    if not _LIB:
        from vibevoice_rocm_amd import _lib as L
        l = L.load()
        L.check(l.vv_init(), "vv_init")
        _LIB.extend((L, l))
    return _LIB


def _inv_freq(d):
    return 1.0 / (1e6 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))


# ---------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------
def _angle(pos, inv_freq):
    """float32(pos) * inv_freq[i], the product formed in fp32 (as the kernel and the reference model do), then widened."""
    return (torch.tensor(float(pos), dtype=torch.float32) * inv_freq.float()).double()


def _rot64(x, ang):
    """half-rotation RoPE in fp64: element i pairs with i + d / 2"""
    h = x.shape[-1] // 2
    c, s = torch.cos(ang), torch.sin(ang)
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def ref_decode_fp64(qkv, kc, vc, lens, inv_freq, heads, detail=False):
    """Decode attention of one layer in fp64.  qkv[R, (heads + 2 kv_heads) d] is the raw projection; kc, vc[rows, kv_heads, s_max, d] is the
    layer's cache as the device received it (fp32 or bf16, widened exactly); row r attends to slots 0 .. lens[r] - 1 of cache row r plus its own
    new token, whose rotated k and v enter unrounded.  Returns out[R, heads, d], and the expected appended slot: rotated k and v [R, kv_heads, d].
    detail=True adds per row (weights w[kv_heads, G, pos + 1] (unnormalised), V[kv_heads, pos + 1, d], scores) for the planted-edge check."""
    R, (_, kvh, _, d) = qkv.shape[0], kc.shape
    G = heads // kvh
    out = torch.empty(R, heads, d, dtype=torch.float64)
    knew = torch.empty(R, kvh, d, dtype=torch.float64)
    vnew = torch.empty(R, kvh, d, dtype=torch.float64)
    rows = []
    for r in range(R):
        pos = int(lens[r])
        ang = _angle(pos, inv_freq)
        row = qkv[r].double()
        q = _rot64(row[: heads * d].view(kvh, G, d), ang)
        kn = _rot64(row[heads * d: (heads + kvh) * d].view(kvh, d), ang)
        vn = row[(heads + kvh) * d:].view(kvh, d)
        K = torch.cat([kc[r, :, :pos].double(), kn[:, None]], 1)
        V = torch.cat([vc[r, :, :pos].double(), vn[:, None]], 1)
        sc = torch.einsum("kgd,ksd->kgs", q, K) / math.sqrt(d)
        w = torch.exp(sc - sc.amax(-1, keepdim=True))
        out[r] = (torch.einsum("kgs,ksd->kgd", w, V) / w.sum(-1, keepdim=True)).reshape(heads, d)
        knew[r], vnew[r] = kn, vn
        rows.append((w, V, sc))
    return (out, knew, vnew, rows) if detail else (out, knew, vnew)


def test_reference_agrees_with_the_fp32_torch_formulation():
    """Guards the reference itself (CPU only): on one small case it must agree with the fp32 torch formulation of
    test_decode_attention_gqa_vs_torch (test_hip_round3.py) to below 1e-6 rel RMS."""
    heads, kvh, d, s_max, lens = 12, 2, 128, 64, (41, 0)
    G, R = heads // kvh, 2
    g = torch.Generator().manual_seed(5)
    kc = torch.randn(R, kvh, s_max, d, generator=g).to(torch.bfloat16)
    vc = torch.randn(R, kvh, s_max, d, generator=g).to(torch.bfloat16)
    qkv = torch.randn(R, (heads + 2 * kvh) * d, generator=g)
    inv_freq = _inv_freq(d)

    def rot(x, pos):
        ang = pos * inv_freq
        c, s_ = torch.cos(ang), torch.sin(ang)
        x1, x2 = x[..., : d // 2], x[..., d // 2:]
        return torch.cat([x1 * c - x2 * s_, x2 * c + x1 * s_], -1)

    want = torch.empty(R, heads, d)
    for r in range(R):
        q = rot(qkv[r, : heads * d].view(heads, d), float(lens[r]))
        kn = rot(qkv[r, heads * d: (heads + kvh) * d].view(kvh, d), float(lens[r]))
        vn = qkv[r, (heads + kvh) * d:].view(kvh, d)
        for h in range(heads):
            kh = torch.cat([kc[r, h // G, : lens[r]].float(), kn[h // G][None]])
            vh = torch.cat([vc[r, h // G, : lens[r]].float(), vn[h // G][None]])
            want[r, h] = torch.softmax((q[h] @ kh.T) / d ** 0.5, -1) @ vh
    got, _, _ = ref_decode_fp64(qkv, kc, vc, lens, inv_freq, heads)
    e = rel_rms(want.numpy(), got.numpy(), "fp32 torch formulation vs the fp64 reference (CPU)")
    assert e < 1e-6, f"reference vs fp32 torch formulation: rel RMS {e:.3e}"


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def split_edges(pos, per_head=(), grouped=()):
    """Cache slots at which a split rule places a boundary: ks and ke - 1 of every live split, plus slot 0 and slot pos - 1.
    per-head kernel: per = ceil(pos / nsplit); grouped kernel: the same rounded up to whole 32-key tiles."""
    e = set()
    if pos > 0:
        e |= {0, pos - 1}
    for n, tile in [(n, 1) for n in per_head] + [(n, 32) for n in grouped]:
        per = -(-pos // n)
        per = -(-per // tile) * tile
        for sp in range(n):
            ks, ke = sp * per, min(pos, sp * per + per)
            if ke > ks:
                e |= {ks, ke - 1}
    return sorted(e)


def batch_edges(pos, stride):
    """Generic kernel: slots around every multiple of its batch stride, plus slot 0 and slot pos - 1."""
    e = {0, pos - 1} if pos > 0 else set()
    for m in range(stride, pos + 2, stride):
        e |= {s for s in (m - 1, m, m + 1) if 0 <= s < pos}
    return sorted(e)


class Case:
    """One call's inputs on the CPU: qkv[R, ld], cache k / v[layers, R + 1, kv_heads, s_max, d] in the cache dtype (NaN behind each addressed
    row's position, the last cache row is addressed by no call and holds random values), and the fp64 reference per layer.

    kind "plain": randn q, k, v.
    kind "planted": at every edge slot (edges_of(pos)) of every (row, KV head) the value row is multiplied by 50 and the key is turned so that
        the group's first q head scores exactly 1.0 on it (randn keys leave the score to chance: with a single q head per group one edge in twenty
        would carry too little weight to be seen) - so dropping or doubling any one of these keys provably moves a (row, head) by >= EDGE_COST.
    kind "peaky": planted, then q times 6 (scores of std 6: the running maximum moves from batch to batch and split to split); row 0's largest
        score sits on its last cached key (the last live split), row 1's on the new token."""

    def __init__(self, heads, kvh, s_max, lens, kind, edges_of=None, d=128, dtype=torch.bfloat16, layers=1, seed=0):
        self.heads, self.kvh, self.s_max, self.lens, self.d, self.dtype, self.layers, self.kind = heads, kvh, s_max, tuple(lens), d, dtype, layers, kind
        self.R, self.G, self.ld = len(lens), heads // kvh, (heads + 2 * kvh) * d
        self.inv_freq = _inv_freq(d)
        R, G, rows = self.R, self.G, self.R + 1
        g = torch.Generator().manual_seed(1000 * seed + 7 * heads + s_max + sum(lens) + len(kind))
        self.qkv = [torch.randn(R, self.ld, generator=g) for _ in range(layers)]
        k = torch.randn(layers, rows, kvh, s_max, d, generator=g)
        v = torch.randn(layers, rows, kvh, s_max, d, generator=g)
        self.edges = [edges_of(p) if kind != "plain" else [] for p in self.lens]
        for l in range(layers):
            qkv = self.qkv[l]
            if kind != "plain":
                for r, pos in enumerate(self.lens):
                    if not self.edges[r]:
                        continue
                    E = torch.tensor(self.edges[r])
                    q0 = _rot64(qkv[r, : heads * d].double().view(kvh, G, d)[:, 0], _angle(pos, self.inv_freq))      # [kvh, d]
                    qn = q0 / q0.norm(dim=-1, keepdim=True)
                    ke = k[l, r][:, E].double()                                                                       # [kvh, |E|, d]
                    along = torch.einsum("ked,kd->ke", ke, qn)
                    want = math.sqrt(d) / q0.norm(dim=-1)                                                             # score 1.0 = q . k / sqrt(d)
                    k[l, r][:, E] = (ke + (want[:, None] - along)[..., None] * qn[:, None]).float()
                    v[l, r][:, E] *= 50.0
            if kind == "peaky":
                qkv[:, : heads * d] *= 6.0
                self._peak(qkv, k[l], row=0, on_new=False)
                if R > 1:
                    self._peak(qkv, k[l], row=1, on_new=True)
        k, v = k.to(dtype), v.to(dtype)
        for r, pos in enumerate(self.lens):
            k[:, r, :, pos:] = float("nan")
            v[:, r, :, pos:] = float("nan")
        self.k, self.v = k, v
        self.has_vt = dtype == torch.bfloat16 and d == 128 and s_max % 32 == 0
        self.vt = vt_tiles(v) if self.has_vt else None
        self._ref = {}

    def _peak(self, qkv, k, row, on_new):
        """put the largest score of every q head of `row` on its last cached key (on_new=False) or on the new token (on_new=True): that key is a
        multiple of the sum of the group's q vectors, sized so that its smallest score over the group's heads is 2 above every other score"""
        heads, kvh, G, d, pos = self.heads, self.kvh, self.G, self.d, self.lens[row]
        assert on_new or pos >= 2
        ang = _angle(pos, self.inv_freq)
        q = qkv[row, : heads * d].double().view(kvh, G, d)
        qr = _rot64(q, ang)
        kn = _rot64(qkv[row, heads * d: (heads + kvh) * d].double().view(kvh, d), ang)
        keys = k[row, :, :pos].to(self.dtype).double()
        sc_cache = torch.einsum("kgd,ksd->kgs", qr, keys) / math.sqrt(d)
        sc_new = torch.einsum("kgd,kd->kg", qr, kn) / math.sqrt(d)
        if on_new:
            others = sc_cache.amax((-1, -2)) if pos else torch.full((kvh,), -1e30, dtype=torch.float64)
            tgt = q.sum(1)                                                   # pre-RoPE: the rotation keeps q . k
            a = torch.einsum("kgd,kd->kg", q, tgt) / math.sqrt(d)
        else:
            others = torch.maximum(sc_cache[..., : pos - 1].amax((-1, -2)), sc_new.amax(-1))
            tgt = qr.sum(1)                                                  # cached keys are stored rotated
            a = torch.einsum("kgd,kd->kg", qr, tgt) / math.sqrt(d)
        assert bool((a > 0).all())
        gamma = (others.clamp_min(0.0) + 2.0) / a.amin(-1)
        if on_new:
            qkv[row, heads * d: (heads + kvh) * d] = (gamma[:, None] * tgt).float().reshape(-1)
        else:
            k[row, :, pos - 1] = (gamma[:, None] * tgt).float()

    def ref(self, layer=0, detail=False):
        """computed once per layer and left unchanged"""
        if layer not in self._ref:
            self._ref[layer] = ref_decode_fp64(self.qkv[layer], self.k[layer], self.v[layer], self.lens, self.inv_freq, self.heads, detail=True)
        return self._ref[layer] if detail else self._ref[layer][:3]

    def assert_edges_carry_weight(self, layer=0):
        """CPU: the fp64 result with any one planted slot removed, and with that slot counted twice, differs from the reference by at least
        EDGE_COST rel RMS in at least one q head of the slot's (row, KV head)."""
        out, _, _, rows = self.ref(layer, detail=True)
        worst = float("inf")
        for r, E in enumerate(self.edges):
            if not E:
                continue
            w, V, _ = rows[r]
            E = torch.tensor(E)
            Z, num = w.sum(-1), torch.einsum("kgs,ksd->kgd", w, V)
            base = num / Z[..., None]
            we = w[:, :, E]                                                        # [kvh, G, |E|]
            wv = we[..., None] * V[:, None, E, :]                                  # [kvh, G, |E|, d]
            for sign in (-1.0, 1.0):
                alt = (num[:, :, None] + sign * wv) / (Z[:, :, None] + sign * we)[..., None]
                rel = (alt - base[:, :, None]).pow(2).mean(-1).sqrt() / base.pow(2).mean(-1).sqrt()[:, :, None]
                worst = min(worst, float(rel.amax(1).min()))                       # best head of the group, worst (KV head, slot)
        assert worst >= EDGE_COST, f"a planted edge moves no head by {EDGE_COST:g}: the weakest moves its best head by {worst:.3e}"
        return worst

    def assert_peaks(self, layer=0):
        """the peaky case's largest scores sit where they were put (checked on the fp64 scores of the cache as the device receives it)"""
        _, _, _, rows = self.ref(layer, detail=True)
        assert bool((rows[0][2].argmax(-1) == self.lens[0] - 1).all()), "row 0: largest score on the last cached key"
        if self.R > 1:
            assert bool((rows[1][2].argmax(-1) == self.lens[1]).all()), "row 1: largest score on the new token"


# ---------------------------------------------------------------------------------------------------------------
# running and checking one call
# ---------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class _Dev:
    """device copies of a case: cache, qkv, lens, RoPE table (from vv_rope_table), NaN-filled outputs"""

    def __init__(self, L, l, case, stream=None):
        c = self.case = case
        self.k, self.v = c.k.cuda(), c.v.cuda()
        self.vt = c.vt.cuda() if c.has_vt else None
        self.qkv = [q.cuda() for q in c.qkv]
        self.lens = torch.tensor(c.lens, dtype=torch.int32).cuda()
        self.inv_freq = c.inv_freq.cuda()
        self.rope = torch.empty(c.R, c.d // 2, 2, device="cuda")
        self.out = [torch.full((c.R, c.heads * c.d), float("nan"), device="cuda") for _ in range(c.layers)]
        self.kv = L.KV(self.k.data_ptr(), self.v.data_ptr(), L.VV_BF16 if c.dtype == torch.bfloat16 else L.VV_F32, c.layers, c.R + 1, c.kvh, c.s_max, c.d,
                       self.vt.data_ptr() if c.has_vt else None)

    def rope_table(self, L, l, stream=None):
        c = self.case
        L.check(l.vv_rope_table(self.lens.data_ptr(), self.inv_freq.data_ptr(), c.R, c.d, self.rope.data_ptr(), stream), "vv_rope_table")

    def decode(self, L, l, layer, ws=None, nsplit=0, part_cap=0, stream=None):
        c = self.case
        a = (self.qkv[layer].data_ptr(), c.ld, c.R, c.heads, C.byref(self.kv), layer, self.rope.data_ptr(), self.lens.data_ptr(), self.out[layer].data_ptr(), c.heads * c.d)
        if ws is None:
            L.check(l.vv_attn_decode(*a, stream), "vv_attn_decode")
        else:
            L.check(l.vv_attn_decode_split(*a, ws[0].data_ptr(), ws[1].data_ptr(), nsplit, part_cap, stream), "vv_attn_decode_split")

    def fetch(self, layer):
        return self.out[layer].cpu(), self.k.cpu(), self.v.cpu(), self.vt.cpu() if self.vt is not None else None


def _workspace(l, R, heads, part_cap):
    """the split route's partials, NaN-filled, and its tickets, zero"""
    part = torch.full((l.vv_attn_decode_part_floats(R, heads, part_cap),), float("nan"), device="cuda")
    return part, torch.zeros(R * heads, dtype=torch.int32, device="cuda")


def _run(case, gqa, nsplit=0, part_cap=0, keys=1024, launched=None, layer=0):
    """one call on fresh device copies.  nsplit = 0: vv_attn_decode; else vv_attn_decode_split with a NaN-filled partials buffer and zeroed tickets,
    which must be zero again afterwards.  launched: the split count the launch must have used - every (row, head, split) writes its
    (m, l, O[128]) record, empty splits included, so exactly R * heads * launched * 130 floats of the buffer are no longer NaN."""
    L, l = _lib()
    dev = _Dev(L, l, case)
    ws = _workspace(l, case.R, case.heads, part_cap) if nsplit else None
    l.vv_tune(b"attn_gqa", gqa)
    l.vv_tune(b"attn_gqa_keys", keys)
    try:
        dev.rope_table(L, l)
        dev.decode(L, l, layer, ws, nsplit, part_cap)
        torch.cuda.synchronize()
    finally:
        l.vv_tune(b"attn_gqa", 1)
        l.vv_tune(b"attn_gqa_keys", 1024)
    if ws is not None:
        assert int(ws[1].abs().sum()) == 0, "tickets are left zero"
        if launched is not None:
            written = int((~torch.isnan(ws[0])).sum())
            assert written == case.R * case.heads * launched * (case.d + 2), f"{written / (case.R * case.heads * (case.d + 2)):g} splits launched, {launched} intended"
    return dev.fetch(layer)


def _check(case, got, tag, layer=0):
    """one call's output against fp64 at both bars, its appended slots (E), and every other byte of the cache"""
    out, k2, v2, vt2 = got
    want, knew, vnew = case.ref(layer)
    R, heads, d = case.R, case.heads, case.d
    assert bool(torch.isfinite(out).all()), f"{tag}: non-finite output"
    o = out.double().view(R, heads, d)
    per_head = (o - want).pow(2).mean(-1).sqrt() / (want.pow(2).mean(-1).sqrt() + 1e-30)
    r_w, h_w = divmod(int(per_head.argmax()), heads)
    e = rel_rms(o.numpy(), want.numpy(), f"{tag}: whole call")
    eh = rel_rms(o[r_w, h_w].numpy(), want[r_w, h_w].numpy(), f"{tag}: worst (row, head) = ({r_w}, {h_w}), position {case.lens[r_w]}")
    print(f"{tag}: global {e:.3e}  worst (row {r_w}, head {h_w}, pos {case.lens[r_w]}) {eh:.3e}")
    assert e < GLOBAL_BAR, f"{tag}: global rel RMS {e:.3e} (bar {GLOBAL_BAR:g})"
    assert eh < HEAD_BAR, f"{tag}: (row {r_w}, head {h_w}) at position {case.lens[r_w]}: rel RMS {eh:.3e} (bar {HEAD_BAR:g})"
    bf = case.dtype == torch.bfloat16
    ek = 0.0
    for r, pos in enumerate(case.lens):
        ek = max(ek, rel_rms(k2[layer, r, :, pos].double().numpy(), knew[r].numpy(), f"{tag}: appended k of row {r}"))
        assert torch.equal(_bits(v2[layer, r, :, pos]), _bits(vnew[r].float().to(case.dtype))), f"{tag}: appended v of row {r} is the value rounded to the cache dtype"
        if vt2 is not None:
            assert torch.equal(_bits(v2[layer, r, :, pos]), _bits(vt2[layer, r, :, pos // 32, :, pos % 32])), f"{tag}: v^T slot of row {r} == v slot"
    assert ek < (K_BF16_BAR if bf else K_F32_BAR), f"{tag}: appended k rel RMS {ek:.3e}"
    for name, before, after in (("k", case.k, k2), ("v", case.v, v2)) + ((("vt", case.vt, vt2),) if vt2 is not None else ()):
        exp = before.clone()
        for r, pos in enumerate(case.lens):
            if name == "vt":
                exp[layer, r, :, pos // 32, :, pos % 32] = after[layer, r, :, pos // 32, :, pos % 32]
            else:
                exp[layer, r, :, pos] = after[layer, r, :, pos]
        assert torch.equal(_bits(exp), _bits(after)), f"{tag}: {name} changed outside the appended slots"
    return e, eh


def _same_appended_bits(case, a, b, tag, layer=0):
    for r, pos in enumerate(case.lens):
        for x, y in ((a[1], b[1]), (a[2], b[2])):
            assert torch.equal(_bits(x[layer, r, :, pos]), _bits(y[layer, r, :, pos])), f"{tag}: row {r}: the two kernels append different k / v bits"
        assert torch.equal(_bits(a[3][layer, r, :, pos // 32, :, pos % 32]), _bits(b[3][layer, r, :, pos // 32, :, pos % 32])), f"{tag}: row {r}: v^T bits differ"


def _lens8(n, s_max):
    """rows with different numbers of empty splits in one launch; the last row appends into the last slot"""
    return (0, 1, n - 1, n, n + 1, 511, 1030, s_max - 1)


# ---------------------------------------------------------------------------------------------------------------
# A. split-key per-head kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsplit", [2, 3, 7, 16])
def test_split_per_head_kernel_vs_fp64(nsplit):
    """vv_attn_decode_split with vv_tune attn_gqa 0 (attn_decode_kernel<8>, keys split over gridDim.z blocks, folded by the block that draws the
    last ticket), bf16 cache, 12 / 2 heads, s_max 2048: one R = 8 call whose rows have 0, 1, nsplit - 1, nsplit, nsplit + 1, 511, 1030 and
    s_max - 1 cached keys (plain and planted data), one R = 1 call, one R = 3 call with peaky data.  The grouped kernel runs the same inputs at
    the same split count: both match fp64 and append the same bits."""
    _need_gpu()
    heads, kvh, s_max = 12, 2, 2048
    edges_of = lambda pos: split_edges(pos, per_head=(nsplit,), grouped=(nsplit,))
    cases = [Case(heads, kvh, s_max, _lens8(nsplit, s_max), "plain", seed=nsplit),
             Case(heads, kvh, s_max, _lens8(nsplit, s_max), "planted", edges_of, seed=nsplit),
             Case(heads, kvh, s_max, (1030,), "plain", seed=nsplit),
             Case(heads, kvh, s_max, (1030, 511, nsplit + 1), "peaky", edges_of, seed=nsplit)]
    cases[1].assert_edges_carry_weight()
    cases[3].assert_peaks()
    for c in cases:
        tag = f"A per-head nsplit={nsplit} R={c.R} {c.kind}"
        a = _run(c, 0, nsplit, nsplit, launched=nsplit)
        _check(c, a, tag)
        b = _run(c, 2, nsplit, nsplit, launched=nsplit)
        _check(c, b, tag + " (grouped kernel, same inputs)")
        _same_appended_bits(c, a, b, tag)


# ---------------------------------------------------------------------------------------------------------------
# B. split-key grouped kernel, every fold width
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,kvh", [(2, 2), (12, 2), (28, 4), (16, 2)])
@pytest.mark.parametrize("ng", [2, 8, 9, 16, 17, 32, 33, 64])
def test_split_grouped_kernel_vs_fp64(ng, heads, kvh):
    """vv_attn_decode_split with attn_gqa 2 (attn_decode_gqa_kernel), G = 1, 6, 7, 8 q heads per KV head.  The launched split count is
    min(max(nsplit, s_max / attn_gqa_keys), part_cap, 64): with s_max 2048 and attn_gqa_keys 32 it is part_cap, which takes the values at which
    the last workgroup's fold changes its compile-time width (J = 2 up to 8 splits, 4 up to 16, 8 up to 32, 16 up to 64) and their neighbours.
    The R = 8 rows have 0, 1, ng - 1, ng, ng + 1, 511, 1030 and s_max - 1 cached keys; plain and planted data.  The per-head kernel (at its own
    cap of 16 splits) must append the same bits."""
    _need_gpu()
    s_max, nsplit = 2048, min(ng, 16)
    edges_of = lambda pos: split_edges(pos, per_head=(nsplit,), grouped=(ng,))
    plain = Case(heads, kvh, s_max, _lens8(ng, s_max), "plain", seed=ng)
    planted = Case(heads, kvh, s_max, _lens8(ng, s_max), "planted", edges_of, seed=ng)
    planted.assert_edges_carry_weight()
    tag = f"B grouped ng={ng} G={heads // kvh}"
    _check(plain, _run(plain, 2, nsplit, ng, keys=32, launched=ng), tag + " plain")
    b = _run(planted, 2, nsplit, ng, keys=32, launched=ng)
    _check(planted, b, tag + " planted")
    a = _run(planted, 0, nsplit, ng, keys=32, launched=nsplit)
    _check(planted, a, tag + " planted (per-head kernel, same inputs)")
    _same_appended_bits(planted, a, b, tag)


# ---------------------------------------------------------------------------------------------------------------
# C. the default rule
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_max", [6144, 6112])
def test_default_rule_vs_fp64(s_max):
    """attn_gqa 1 (as shipped) on both sides of kv_heads * s_max >= 12288 (2 KV heads: s_max 6144 takes the grouped kernel, 6112 the per-head one;
    which one ran is not observed - both must match fp64), with vv_llm_forward's split count min(16, ceil(s_max / 512)) and its partials capacity
    of 128 splits, at R = 2 (plain) and R = 8 (planted), positions up to s_max - 1.  Forcing either kernel appends the same bits."""
    _need_gpu()
    heads, kvh = 12, 2
    nsplit, cap = min(16, -(-s_max // 512)), 128
    edges_of = lambda pos: split_edges(pos, per_head=(nsplit,), grouped=(nsplit,))
    c2 = Case(heads, kvh, s_max, (s_max - 1, 1030), "plain", seed=3)
    c8 = Case(heads, kvh, s_max, (0, 1, nsplit - 1, nsplit + 1, 511, 3000, s_max - 2, s_max - 1), "planted", edges_of, seed=3)
    c8.assert_edges_carry_weight()
    for c in (c2, c8):
        tag = f"C default rule s_max={s_max} R={c.R} {c.kind}"
        _check(c, _run(c, 1, nsplit, cap, launched=nsplit), tag)
        a = _run(c, 0, nsplit, cap, launched=nsplit)
        b = _run(c, 2, nsplit, cap, launched=nsplit)
        _check(c, a, tag + " (per-head forced)")
        _check(c, b, tag + " (grouped forced)")
        _same_appended_bits(c, a, b, tag)


# ---------------------------------------------------------------------------------------------------------------
# D. workspace reuse as the LLM step does it
# ---------------------------------------------------------------------------------------------------------------
def _reuse_case():
    edges_of = lambda pos: split_edges(pos, per_head=(4, 9), grouped=(4, 9))
    return Case(12, 2, 2048, (1030, 511, 2047), "planted", edges_of, layers=2, seed=11)


@pytest.mark.parametrize("gqa,nsplit,cap,keys,launched", [(0, 4, 4, 1024, 4), (2, 4, 9, 32, 9)], ids=["per_head", "grouped"])
def test_workspace_reused_across_layers(gqa, nsplit, cap, keys, launched):
    """vv_llm_forward zeroes the tickets once per step and hands every layer the same partials buffer: two calls, layer 0 then layer 1 (different
    cache contents and projections), on one workspace with nothing re-zeroed in between - each must match its own reference."""
    _need_gpu()
    L, l = _lib()
    c = _reuse_case()
    dev = _Dev(L, l, c)
    ws = _workspace(l, c.R, c.heads, cap)
    l.vv_tune(b"attn_gqa", gqa)
    l.vv_tune(b"attn_gqa_keys", keys)
    try:
        dev.rope_table(L, l)
        dev.decode(L, l, 0, ws, nsplit, cap)
        dev.decode(L, l, 1, ws, nsplit, cap)
        torch.cuda.synchronize()
    finally:
        l.vv_tune(b"attn_gqa", 1)
        l.vv_tune(b"attn_gqa_keys", 1024)
    assert int(ws[1].abs().sum()) == 0, "tickets are left zero"
    assert int((~torch.isnan(ws[0])).sum()) == c.R * c.heads * launched * 130
    k2, v2, vt2 = dev.k.cpu(), dev.v.cpu(), dev.vt.cpu()
    for layer in (0, 1):
        want, knew, vnew = c.ref(layer)
        out = dev.out[layer].cpu()
        assert bool(torch.isfinite(out).all())
        o = out.double().view(c.R, c.heads, c.d)
        tag = f"D reuse {'grouped' if gqa else 'per-head'} layer {layer}"
        e = rel_rms(o.numpy(), want.numpy(), tag)
        ph = (o - want).pow(2).mean(-1).sqrt() / want.pow(2).mean(-1).sqrt()
        r_w, h_w = divmod(int(ph.argmax()), c.heads)
        eh = rel_rms(o[r_w, h_w].numpy(), want[r_w, h_w].numpy(), f"{tag}: worst (row, head) = ({r_w}, {h_w})")
        print(f"{tag}: global {e:.3e} worst head {eh:.3e}")
        assert e < GLOBAL_BAR and eh < HEAD_BAR, f"{tag}: global {e:.3e}, worst (row, head) {eh:.3e}"
        for r, pos in enumerate(c.lens):
            assert rel_rms(k2[layer, r, :, pos].double().numpy(), knew[r].numpy()) < K_BF16_BAR
            assert torch.equal(_bits(v2[layer, r, :, pos]), _bits(vnew[r].float().to(c.dtype)))
            assert torch.equal(_bits(v2[layer, r, :, pos]), _bits(vt2[layer, r, :, pos // 32, :, pos % 32]))


@pytest.mark.parametrize("gqa,nsplit,cap,keys", [(0, 4, 4, 1024), (2, 4, 9, 32)], ids=["per_head", "grouped"])
def test_workspace_reused_in_a_replayed_graph(gqa, nsplit, cap, keys):
    """The same two calls and the RoPE table of the lens they read, captured between vv_graph_begin and vv_graph_end and replayed three times on
    one workspace whose tickets were zeroed once, before the capture; the cache is restored between replays.  Every replay matches fp64 and
    gives the bits of the first; the tickets end at zero."""
    _need_gpu()
    L, l = _lib()
    c = _reuse_case()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        dev = _Dev(L, l, c)
        ws = _workspace(l, c.R, c.heads, cap)
        k0, v0, vt0 = dev.k.clone(), dev.v.clone(), dev.vt.clone()
    st.synchronize()
    torch.cuda.synchronize()
    sp = st.cuda_stream
    ge = C.c_void_p()
    l.vv_tune(b"attn_gqa", gqa)
    l.vv_tune(b"attn_gqa_keys", keys)
    try:
        L.check(l.vv_graph_begin(sp), "vv_graph_begin")
        try:
            dev.rope_table(L, l, sp)
            dev.decode(L, l, 0, ws, nsplit, cap, sp)
            dev.decode(L, l, 1, ws, nsplit, cap, sp)
        finally:
            rc = l.vv_graph_end(sp, C.byref(ge))
        L.check(rc, "vv_graph_end")
    finally:
        l.vv_tune(b"attn_gqa", 1)
        l.vv_tune(b"attn_gqa_keys", 1024)
    try:
        outs = []
        for i in range(3):
            with torch.cuda.stream(st):
                dev.k.copy_(k0); dev.v.copy_(v0); dev.vt.copy_(vt0)
                for o in dev.out:
                    o.fill_(float("nan"))
                L.check(l.vv_graph_launch(ge, sp), "vv_graph_launch")
            st.synchronize()
            assert int(ws[1].abs().sum()) == 0, f"replay {i}: tickets are left zero"
            outs.append([o.cpu() for o in dev.out])
    finally:
        l.vv_graph_destroy(ge)
    for layer in (0, 1):
        want = c.ref(layer)[0]
        o = outs[0][layer].double().view(c.R, c.heads, c.d)
        assert bool(torch.isfinite(o).all())
        tag = f"D graph replay {'grouped' if gqa else 'per-head'} layer {layer}"
        e = rel_rms(o.numpy(), want.numpy(), tag)
        ph = (o - want).pow(2).mean(-1).sqrt() / want.pow(2).mean(-1).sqrt()
        r_w, h_w = divmod(int(ph.argmax()), c.heads)
        eh = rel_rms(o[r_w, h_w].numpy(), want[r_w, h_w].numpy(), f"{tag}: worst (row, head) = ({r_w}, {h_w})")
        assert e < GLOBAL_BAR and eh < HEAD_BAR, f"{tag}: global {e:.3e}, worst (row, head) {eh:.3e}"
        for i in (1, 2):
            assert torch.equal(outs[i][layer].view(torch.int32), outs[0][layer].view(torch.int32)), f"{tag}: replay {i} differs from the first"


# ---------------------------------------------------------------------------------------------------------------
# F. the generic kernel
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [(torch.float32, 64), (torch.float32, 128), (torch.bfloat16, 64)], ids=["f32_d64", "f32_d128", "bf16_d64"])
def test_generic_kernel_vs_fp64(dtype, d):
    """vv_attn_decode on the caches the head_dim-128 bf16 kernels refuse (attn_fused_kernel: 16 waves, KPW = 64 / (d / EPL) keys per wave and
    step, a batch of stride = 16 * KPW * 4 keys per buffer, two buffers alternating): positions on both sides of one lane group, one wave
    step, one, two and three strides, and the last slot of the cache; 4 / 2 heads, R = 2, layer 1 of 2, plain data and data planted around every
    multiple of the stride.  The appended v is exact, the appended k carries fp32 arithmetic (fp32 cache) or one bf16 rounding (bf16 cache)."""
    _need_gpu()
    epl = 4 if dtype == torch.float32 else 8
    kpw = 64 // (d // epl)
    stride = 16 * kpw * 4
    s_max = 3 * stride + 7
    pos = [0, 1, kpw - 1, kpw, stride - 1, stride, stride + 1, 2 * stride, 2 * stride + 1, 3 * stride + 5, s_max - 1, 2 * stride - 1]
    assert (kpw, stride) == {(torch.float32, 64): (4, 256), (torch.float32, 128): (2, 128), (torch.bfloat16, 64): (8, 512)}[(dtype, d)]
    edges_of = lambda p: batch_edges(p, stride)
    for i in range(0, len(pos), 2):
        for kind in ("plain", "planted"):
            c = Case(4, 2, s_max, (pos[i], pos[i + 1]), kind, edges_of, d=d, dtype=dtype, layers=2, seed=i)
            if kind == "planted" and max(c.lens) > 0:
                c.assert_edges_carry_weight(1)
            _check(c, _run(c, 1, layer=1), f"F generic {'f32' if dtype == torch.float32 else 'bf16'} d={d} lens={c.lens} {kind}", layer=1)


# ---------------------------------------------------------------------------------------------------------------
# G. the RoPE table
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [128, 64])
def test_rope_table_vs_fp64(d):
    """vv_rope_table[r][i] = {cos, sin}(float(lens[r]) * inv_freq[i]) against fp64 cos / sin of the same fp32 product, base 1e6, positions up to
    100 000 (long-form decode reaches 65 535).  Absolute bound 4 x 2^-23: cosf / sinf are correct to a few ulp of values in [-1, 1]; a fast-math
    or hardware-intrinsic path would show as ~1e-3 at the large positions."""
    _need_gpu()
    L, l = _lib()
    lens = torch.tensor([0, 1, 2, 1023, 4096, 32767, 65535, 100000], dtype=torch.int32)
    inv_freq = _inv_freq(d)
    table = torch.full((8, d // 2, 2), float("nan"), device="cuda")
    ld, fd = lens.cuda(), inv_freq.cuda()
    L.check(l.vv_rope_table(ld.data_ptr(), fd.data_ptr(), 8, d, table.data_ptr(), None), "vv_rope_table")
    torch.cuda.synchronize()
    got = table.cpu().double()
    ang = (lens.float()[:, None] * inv_freq[None, :]).double()           # the product in fp32
    want = torch.stack([torch.cos(ang), torch.sin(ang)], -1)
    assert bool(torch.isfinite(got).all())
    err = (got - want).abs()
    rel_rms(got.numpy(), want.numpy(), f"G rope table d={d} (rel RMS; max abs error {float(err.max()):.3e})")
    worst = int(err.amax((1, 2)).argmax())
    print(f"G rope table d={d}: max abs error {float(err.max()):.3e} at position {int(lens[worst])}")
    assert float(err.max()) <= ROPE_BAR, f"rope table d={d}: max abs error {float(err.max()):.3e} at position {int(lens[worst])} (bound {ROPE_BAR:.2e})"
