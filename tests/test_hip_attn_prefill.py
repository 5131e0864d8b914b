"""Prompt attention (vv_attn) and the RoPE / KV store (vv_rope_store) against fp64 references - all `-m gpu`, all through the C ABI, no engine
and no model weights.  Every parity case first asks `vv_attn_route` which kernel its arguments take and asserts the one it means to test.

  A  the matrix-core kernel (attn_prefill_mfma): prompts (R rows at pos0 .. pos0 + R - 1 of one cache row) whose last key tile ends on every
     residue of 4 (the `left` masks of the scrub) and on 0 / 1 / 31 of 32, and row-batched calls: non-monotone lens, three cache rows in one
     query tile (one far shorter than the riding lanes' lens), one cache row named from two query tiles, 40 rows on 40 cache rows
  B  the grouped kernel, all 12 instantiations (NQ 2 / 6 / 7 x bf16 / fp32 x head_dim 128 / 64), 24 rows whose key counts sit at and around
     every multiple of the kernel's stride up to three double-strides
  C  the per-head kernel: R = 1 / 3 / 7, GQA ratios 1 / 3 / 4, vv_tune("attn_group", 0), an ld_qkv that is no multiple of 4, bf16 and fp32,
     head_dim 128 / 64 / 16
  D  the fall-backs the route decides: vt set but R = 15, s_max % 32 != 0, head_dim 64, ldo % 4 != 0; NQ * ng > 256
  E  vv_rope_store directly: q in place, rotated k, v and v^T slots, and every other byte of qkv and of the cache
  F  vv_rope_table -> vv_rope_store -> vv_attn for 77 prompt rows, as one call and as two chunks whose edge lies inside a 32-key tile

References (plain torch fp64 on the cache as the device received it; they know nothing of tiles): `ref_prompt_fp64`, and for the matrix-core
kernel `ref_prompt_contract`, the same with q replaced by what that kernel documents it uses, bf16_rne(fp32(q) * fp32(rsqrt(128) * log2 e)),
scores in the log2 domain - which leaves the kernel's bf16 rounding of P as the only modelled-away difference.
"planted" inputs: the first q head of every GQA group is corrected (minimum norm) so that it scores max(ln n, 1) on each of its row's edge
slots (keys are shared by the query rows of a prompt, so the planting is done on the query).  A CPU check shows that dropping or doubling
any one of those keys moves that (row, head) by >= EDGE_COST = 5e-2 in every planted case; the weakest planted key of the file costs 6.0e-2
(group A 1.3e-1, B 8.9e-2, C 9.2e-2, D 6.0e-2).  Below head_dim 128 a row plants only its highest stride boundaries (stride_edges).
"peaky": planted, then q x 6 (scores of std 6: the running maximum moves; no edge-cost claim).

Bars.  Grouped and per-head kernels (fp32 arithmetic) against fp64: 2e-4 per call, 1e-3 for the worst (row, head), as for decode attention.
Matrix-core kernel: worst (row, head) against the contract reference 5e-3 = EDGE_COST / 10 (each weight is rounded to bf16, 2^-8 relative at
most and about 1.6e-3 rms, while the weights are summed unrounded; the CPU emulation of that rounding predicted about 2e-3); per-call
rel RMS against pure fp64 5e-3 on plain and planted data (on peaky data the Q rounding moves scores of std 6 and only the contract
comparison is judged).

Measured on the MI355X, largest value over the group's calls (profiles/attn_prefill_parity.txt):
  A  matrix-core, worst (row, head) vs contract      plain 2.43e-3, planted 2.24e-3, peaky 1.94e-3    bar 5e-3 = 2.06 x the largest
     matrix-core, per call vs fp64                   plain 2.35e-3, planted 2.71e-3                    bar 5e-3 (peaky, not judged: 5.4e-3;
                                                                                                       one (row, head) vs fp64: 2.9e-2)
  B  grouped kernel, global / worst (row, head)      plain 9.5e-8 / 3.7e-7, planted 1.3e-7 / 5.1e-7, peaky 3.7e-7 / 2.1e-6
  C  per-head kernel, global / worst (row, head)     plain 1.5e-7 / 4.3e-7, planted 1.5e-7 / 5.2e-7
  D  fall-backs                                      grouped 1.1e-7 / 4.0e-7, per-head (NQ * ng = 384) 1.1e-7 / 5.0e-7
  E  rope store                                      q in place 6.2e-8 (bar 9.5e-7), stored k fp32 5.5e-8, bf16 2.2e-3 (one rounding, bar 4e-3);
                                                     v, v^T and every other byte exact
  F  one call and two chunks                         worst (row, head) vs contract 2.13e-3, per call vs fp64 1.63e-3, the same in both runs:
                                                     outputs and caches of the two runs are bit-identical
The fp32 kernels are 480 x (worst (row, head), grouped, peaky) and more below their bars.  The matrix-core kernel's worst (row, head), 2.43e-3
(28 / 4 heads, R = 77: row 9, 10 keys), leaves the factor of two the bar was set with and no more: a change that adds rounding there will show.
"""
import ctypes as C
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from conftest import rel_rms, vt_tiles

pytestmark = pytest.mark.gpu

GLOBAL_BAR = 2e-4        # grouped / per-head kernels: rel RMS of a whole call against fp64
HEAD_BAR = 1e-3          # grouped / per-head kernels: rel RMS of the worst (row, head) of a call against fp64
EDGE_COST = 5e-2         # what one dropped / doubled planted key must cost its (row, head) (checked on the CPU for every planted case)
MFMA_HEAD_BAR = 5e-3     # matrix-core kernel: worst (row, head) against the contract reference; must stay <= EDGE_COST / 10
MFMA_GLOBAL_BAR = 5e-3   # matrix-core kernel: rel RMS of a whole call against pure fp64 (plain and planted data)
K_BF16_BAR = 4e-3        # stored rotated key against the unrounded fp64 one: one bf16 rounding, at most 2^-8 = 3.9e-3 relative per element
K_F32_BAR = 16 * 2.0 ** -24   # fp32 rotation on a cos / sin table correct to a few ulp: two products and one sum in fp32 - 16 half-ulps is a generous ceiling
assert MFMA_HEAD_BAR <= EDGE_COST / 10

SENT32 = 0x7FC0BEEF      # NaN bit patterns: pad columns, unwritten outputs, untouched cache bytes
SENT16 = 0x7FC5
BF16, F32 = torch.bfloat16, torch.float32


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


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _sentinel(shape, dtype=F32):
    if dtype == BF16:
        return torch.full(shape, SENT16, dtype=torch.int16).view(BF16)
    return torch.full(shape, SENT32, dtype=torch.int32).view(F32)


# ---------------------------------------------------------------------------------------------------------------
# the references
# ---------------------------------------------------------------------------------------------------------------
def _angle(pos, inv_freq):
    """float32(pos) * inv_freq[i], the product formed in fp32 (as vv_rope_table does), then widened."""
    return (torch.tensor(float(pos), dtype=torch.float32) * inv_freq.float()).double()


def _rot64(x, ang):
    """half-rotation RoPE in fp64: element i pairs with i + d / 2"""
    h = x.shape[-1] // 2
    c, s = torch.cos(ang), torch.sin(ang)
    x1, x2 = x[..., :h], x[..., h:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def _softmax_rows(q, kc, vc, lens, cache_rows, heads, log2, detail):
    R, (_, kvh, _, d) = q.shape[0], kc.shape
    G = heads // kvh
    out = torch.empty(R, heads, d, dtype=torch.float64)
    rows = []
    for r in range(R):
        n = int(lens[r]) + 1
        c = r if cache_rows is None else int(cache_rows[r])
        K, V = kc[c, :, :n].double(), vc[c, :, :n].double()
        sc = torch.einsum("kgd,ksd->kgs", q[r].double().view(kvh, G, d), K)
        if not log2:
            sc = sc / math.sqrt(d)
        z = sc - sc.amax(-1, keepdim=True)
        w = torch.exp2(z) if log2 else torch.exp(z)
        out[r] = (torch.einsum("kgs,ksd->kgd", w, V) / w.sum(-1, keepdim=True)).reshape(heads, d)
        rows.append((w, V))
    return (out, rows) if detail else out


def ref_prompt_fp64(q, kc, vc, lens, cache_rows, heads, detail=False):
    """Prompt attention of one layer in fp64.  q[R, heads, d]; kc, vc[rows, kv_heads, s_max, d] is the layer's cache as the device received it
    (fp32 or bf16, widened exactly); row r is a softmax over slots 0 .. lens[r] of cache row cache_rows[r] (None: r).  Returns out[R, heads, d];
    detail=True adds per row the unnormalised weights w[kv_heads, G, n] and V[kv_heads, n, d] for the planted-edge check."""
    return _softmax_rows(q, kc, vc, lens, cache_rows, heads, False, detail)


def contract_q(q, d):
    """what the matrix-core kernel documents it uses for q: bf16_rne(fp32(q) * fp32(rsqrt(d) * log2 e)), the factor and the product formed in fp32"""
    qsc = torch.rsqrt(torch.tensor(float(d), dtype=torch.float32)) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    return (q.float() * qsc).to(BF16)


def ref_prompt_contract(q, kc, vc, lens, cache_rows, heads):
    """ref_prompt_fp64 with q replaced by contract_q and the scores taken in the log2 domain: everything else (no tiles, no running maximum, no
    rounding of the weights) as above"""
    return _softmax_rows(contract_q(q, kc.shape[-1]), kc, vc, lens, cache_rows, heads, True, False)


def ref_rope_store_fp64(qkv, lens, inv_freq, heads, kvh, d):
    """what vv_rope_store leaves: rotated q[R, heads, d], rotated k[R, kv_heads, d], v[R, kv_heads, d] (unchanged), all fp64"""
    R = qkv.shape[0]
    x = qkv.double()
    ang = torch.stack([_angle(int(p), inv_freq) for p in lens])[:, None, :]
    q = _rot64(x[:, : heads * d].view(R, heads, d), ang)
    k = _rot64(x[:, heads * d: (heads + kvh) * d].view(R, kvh, d), ang)
    return q, k, x[:, (heads + kvh) * d: (heads + 2 * kvh) * d].view(R, kvh, d)


def test_references_agree_with_the_fp32_torch_formulation():
    """Guards the references themselves (CPU only): on one small case ref_prompt_fp64 agrees with the fp32 torch formulation of
    test_prompt_attention_vs_torch (test_hip_parity.py) to below 1e-6 rel RMS, and the log2-domain path of the contract reference, fed the
    unrounded q * rsqrt(d) * log2 e, agrees with it to fp64 rounding."""
    heads, kvh, d, R, pos0 = 12, 2, 128, 21, 5
    g = torch.Generator().manual_seed(9)
    s_max = pos0 + R + 3
    kc = torch.randn(2, kvh, s_max, d, generator=g).to(BF16)
    vc = torch.randn(2, kvh, s_max, d, generator=g).to(BF16)
    q = torch.randn(R, heads, d, generator=g)
    lens = torch.arange(pos0, pos0 + R, dtype=torch.int32)
    want = torch.empty(R, heads, d)
    for h in range(heads):
        kh, vh = kc[1, h // (heads // kvh)].float(), vc[1, h // (heads // kvh)].float()
        sc = (q[:, h] @ kh.T) / d ** 0.5
        sc = sc.masked_fill(torch.arange(s_max)[None, :] > lens[:, None], float("-inf"))
        want[:, h] = torch.softmax(sc, -1) @ vh
    crows = [1] * R
    got = ref_prompt_fp64(q, kc, vc, lens, crows, heads)
    e = rel_rms(want.numpy(), got.numpy(), "fp32 torch formulation vs the fp64 reference (CPU)")
    assert e < 1e-6, f"reference vs fp32 torch formulation: rel RMS {e:.3e}"
    got2 = _softmax_rows(q.double() * (math.log2(math.e) / math.sqrt(d)), kc, vc, lens, crows, heads, True, False)
    e2 = rel_rms(got2.numpy(), got.numpy(), "log2-domain path vs the fp64 reference (CPU)")
    assert e2 < 1e-12, f"log2-domain path vs the fp64 reference: rel RMS {e2:.3e}"


# ---------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------
def mfma_edges(n):
    """matrix-core kernel, a row of n keys: slot 0, the last and the one before, the first key of the last 32-key tile and the key before it,
    and the first tile boundary (31, 32)"""
    t = 32 * ((n - 1) // 32)
    return sorted(s for s in {0, n - 1, n - 2, t, t - 1, 31, 32} if 0 <= s < n)


def stride_edges(stride, d=128):
    """grouped / per-head kernels, a row of n keys: the first and the last key and the keys either side of each multiple of the stride below n.
    A query of head_dim d cannot hold many keys at score ln n without also raising its score on chance keys (its correction has |E| ln^2 n of
    energy spread over d dimensions): below head_dim 128 a row plants at most d / 8 - 2 of these slots, the pair at the highest multiple
    first, then the last and the first key, then the pairs at lower multiples.  The key counts of a call sit just above every multiple of the
    stride, so every boundary is the highest one of some row and is planted there."""
    budget = 14 if d >= 128 else max(d // 8 - 2, 2)

    def of(n):
        pairs = [s for m in range(stride * ((n - 1) // stride), 0, -stride) for s in (m, m - 1)]
        return sorted(list(dict.fromkeys(pairs[:2] + [n - 1, 0] + pairs[2:]))[:budget])
    return of


def kernel_stride(dtype, d):
    """keys per block step of the grouped and per-head kernels: 4 waves x KPW = 64 / G keys, G = d / EPL lanes per key (EPL: 16 bytes of cache)"""
    return 4 * (64 // (d // (4 if dtype == F32 else 8)))


class Case:
    """One vv_attn call's inputs on the CPU.  Cache k / v[2, rows, kv_heads, s_max, d] in the cache dtype; the call addresses layer 1; rows is
    one more than any row the call names, and every row the call does not name holds random values.  Of a named cache row, slots up to its
    written length (the largest lens + 1 of the query rows that name it) are random, every slot behind it holds NaN - in k, v and vt.
    qkv[R, ld_qkv] and out[R, ldo] carry pad columns that hold a NaN sentinel (SENT32); out is sentinel everywhere before the call.

    kind "plain": randn q, k, v.
    kind "planted": per (row, KV head) the group's first q head gets the minimum-norm correction that makes it score max(ln n, 1) on every slot
        of edges_of(n), n = lens[r] + 1 (keys are shared by the query rows of a prompt, so the planting is done on the query).
    kind "peaky": planted, then q x 6."""

    def __init__(self, name, route, heads, kvh, lens, crows, kind, edges_of, d=128, dtype=BF16, vt=False, s_max=None, pad_q=4, pad_o=4, attn_group=1):
        self.name, self.route, self.heads, self.kvh, self.kind, self.d, self.dtype, self.attn_group = name, route, heads, kvh, kind, d, dtype, attn_group
        self.lens, self.crows = [int(x) for x in lens], None if crows is None else [int(c) for c in crows]
        R, G = len(self.lens), heads // kvh
        self.R, self.G = R, G
        named = list(range(R)) if crows is None else self.crows
        self.n_rows = max(named) + 2
        written = {}
        for r, c in enumerate(named):
            written[c] = max(written.get(c, 0), self.lens[r] + 1)
        n_max = max(written.values())
        self.s_max = s_max if s_max is not None else (-(-n_max // 32) * 32 if vt else n_max + 3)
        assert n_max <= self.s_max, "every addressed slot lies inside the cache"
        assert not vt or self.s_max % 32 == 0 or route != "attn_prefill_mfma", "the matrix-core kernel reads whole 32-key tiles"
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        k = torch.randn(2, self.n_rows, kvh, self.s_max, d, generator=g).to(dtype)
        v = torch.randn(2, self.n_rows, kvh, self.s_max, d, generator=g).to(dtype)
        q = torch.randn(R, heads, d, generator=g)
        self.edges = [edges_of(n + 1) if kind != "plain" else [] for n in self.lens]
        if kind != "plain":
            for r, E in enumerate(self.edges):
                n = self.lens[r] + 1
                t = max(math.log(n), 1.0) * math.sqrt(d)
                KE = k[1, named[r]][:, torch.tensor(E)].double()                             # [kvh, |E|, d], as the device will hold them
                q0 = q[r].view(kvh, G, d)[:, 0].double()                                     # [kvh, d]
                resid = t - torch.einsum("ked,kd->ke", KE, q0)
                delta = torch.einsum("ked,ke->kd", KE, torch.linalg.solve(KE @ KE.transpose(1, 2), resid))
                q[r].view(kvh, G, d)[:, 0] = (q0 + delta).float()
        if kind == "peaky":
            q *= 6.0
        for c, n in written.items():
            k[1, c, :, n:] = float("nan")
            v[1, c, :, n:] = float("nan")
        self.q, self.k, self.v = q, k, v
        self.vt = None
        if vt:       # a cache the matrix-core kernel refuses for its s_max never has its vt read: all NaN
            self.vt = vt_tiles(v) if self.s_max % 32 == 0 else torch.full_like(v, float("nan"))
        nat = (heads + 2 * kvh) * d
        self.ld_qkv, self.ldo = nat + pad_q, heads * d + pad_o
        self.qkv = _sentinel((R, self.ld_qkv))
        self.qkv[:, : heads * d] = q.view(R, heads * d)
        self.qkv[:, heads * d: nat] = torch.randn(R, nat - heads * d, generator=g)           # the k / v sections: vv_attn does not read them
        self._ref = None

    def ref(self, detail=False):
        """computed once and left unchanged"""
        if self._ref is None:
            self._ref = ref_prompt_fp64(self.q, self.k[1], self.v[1], self.lens, self.crows, self.heads, detail=True)
        return self._ref if detail else self._ref[0]

    def edge_cost(self):
        """CPU: the fp64 result of the planted (row, head) with any one planted slot removed, and with that slot counted twice, differs from the
        reference by at least this much (rel RMS); a row's only key is exempt from the doubling half (a lone key's softmax does not change)"""
        out, rows = self.ref(detail=True)
        worst = float("inf")
        for r, E in enumerate(self.edges):
            w, V = rows[r]
            w, E = w[:, 0], torch.tensor(E)                                                  # the planted head of every group: [kvh, n]
            Z, num = w.sum(-1), torch.einsum("ks,ksd->kd", w, V)
            base = num / Z[:, None]
            we = w[:, E]                                                                     # [kvh, |E|]
            wv = we[..., None] * V[:, E, :]                                                  # [kvh, |E|, d]
            for sign in (-1.0, 1.0):
                if w.shape[-1] == 1:
                    if sign > 0:
                        continue
                    alt = torch.zeros_like(wv)                                               # the only key removed: nothing is left
                else:
                    alt = (num[:, None] + sign * wv) / (Z[:, None] + sign * we)[..., None]
                rel = (alt - base[:, None]).pow(2).mean(-1).sqrt() / base.pow(2).mean(-1).sqrt()[:, None]
                worst = min(worst, float(rel.min()))
        return worst


def _prompt(heads, kvh, R, pos0, kind):
    return Case(f"A {heads}/{kvh} R={R} pos0={pos0} {kind}", "attn_prefill_mfma", heads, kvh, range(pos0, pos0 + R), [1] * R, kind, mfma_edges, vt=True)


# (R, pos0) of group A.  (pos0 + R) mod 4 sets the `left` masks of the last-tile scrub, (pos0 + R) mod 32 where the last tile ends:
#   16/0 -> 16, 17/31 -> 48, 32/0 -> 32 (mod 32 = 0), 64/500 -> 564: mod 4 = 0        77/0 -> 77, 17/16 -> 33 (mod 32 = 1): mod 4 = 1
#   18/16 -> 34: mod 4 = 2                                                             33/130 -> 163, 31/32 -> 63 (mod 32 = 31), 40/3 -> 43: mod 4 = 3
# (17/16 and 18/16 are there for mod 32 = 1 and mod 4 = 2 on a prompt; the per-row key counts of case (d) reach both again.)
A_PROMPTS = [(16, 0), (17, 31), (32, 0), (33, 130), (31, 32), (77, 0), (64, 500), (40, 3), (17, 16), (18, 16)]
assert {(p + R) % 4 for R, p in A_PROMPTS} == {0, 1, 2, 3} and {0, 1, 31} <= {(p + R) % 32 for R, p in A_PROMPTS}
D_COUNTS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65]


def _specs_a():
    s = {}
    for R, pos0 in A_PROMPTS:
        for kind in ("plain", "planted", "peaky"):
            s[f"12x2-R{R}-p{pos0}-{kind}"] = functools.partial(_prompt, 12, 2, R, pos0, kind)
    for heads, kvh, prompts in ((28, 4, [(77, 0), (64, 500), (40, 3)]), (4, 2, [(16, 0), (33, 130), (31, 32)])):
        for R, pos0 in prompts:
            for kind in ("plain", "planted"):
                s[f"{heads}x{kvh}-R{R}-p{pos0}-{kind}"] = functools.partial(_prompt, heads, kvh, R, pos0, kind)
    perm = torch.randperm(32, generator=torch.Generator().manual_seed(1)).tolist()
    batched = {
        # (a) non-monotone lens within one 32-query tile, one cache row
        "a-nonmonotone": ([10 + p for p in perm], [0] * 32),
        # (b) three cache rows inside one tile; row 2 holds 3 .. 6 keys while the lanes that ride along its pass have lens of 60 .. 100
        "b-three-rows": ([(2 + r // 3 % 4) if r % 3 == 2 else 60 + (r * 7) % 41 for r in range(32)], [r % 3 for r in range(32)]),
        # (c) cache row 0 named from query tiles 0 and 1, cache row 1 from both as well
        "c-two-tiles": ([20 + (r * 5) % 48 for r in range(48)], [0 if r < 16 or r >= 32 else 1 for r in range(48)]),
        # (d) 40 rows, each on its own cache row and its own key count
        "d-own-rows": ([D_COUNTS[r % len(D_COUNTS)] - 1 for r in range(40)], list(range(40))),
    }
    for key, (lens, crows) in batched.items():
        for kind in ("plain", "planted"):
            s[f"{key}-{kind}"] = functools.partial(Case, f"A {key} {kind}", "attn_prefill_mfma", 12, 2, lens, crows, kind, mfma_edges, vt=True)
    return s


def stride_counts(s):
    """24 key counts: 1, and at and around every multiple of the stride s (and so of 2 s) up to three double-strides, in a fixed shuffled order"""
    counts = [1, 2, 3, 5, 2 * s + s // 2, 6 * s + 5] + [m + o for m in range(s, 6 * s + 1, s) for o in (-1, 0, 1)]
    assert len(counts) == 24
    order = torch.randperm(24, generator=torch.Generator().manual_seed(s)).tolist()
    return [counts[i] for i in order]


def _dt(dtype):
    return "bf16" if dtype == BF16 else "f32"


def _specs_b():
    s = {}
    for dtype in (BF16, F32):
        for d in (128, 64):
            G = d // (4 if dtype == F32 else 8)
            stride = kernel_stride(dtype, d)
            for nq in (2, 6, 7):
                route = f"attn_group<{_dt(dtype)},nq{nq},g{G if d == 128 else 0}>"
                kinds = ("plain", "planted") + (("peaky",) if dtype == BF16 and d == 128 else ())
                for kind in kinds:
                    counts = stride_counts(stride)
                    s[f"{_dt(dtype)}-d{d}-nq{nq}-{kind}"] = functools.partial(
                        Case, f"B {_dt(dtype)} d={d} nq={nq} {kind}", route, 2 * nq, 2, [n - 1 for n in counts], [(5 * r + 1) % 3 for r in range(24)], kind,
                        stride_edges(stride, d), d=d, dtype=dtype)
    return s


def _specs_c():
    s = {}
    #        id                 heads kvh R  dtype d   attn_group pad_q
    rows = [("R1",              12, 2, 1,  BF16, 128, 1, 4),
            ("R3",              12, 2, 3,  BF16, 128, 1, 4),
            ("R7",              12, 2, 7,  BF16, 128, 1, 4),
            ("R7-f32",          12, 2, 7,  F32,  128, 1, 4),
            ("ratio1",          2,  2, 24, BF16, 128, 1, 4),
            ("ratio3",          6,  2, 24, BF16, 128, 1, 4),
            ("ratio4",          8,  2, 24, F32,  128, 1, 4),
            ("tune-off",        12, 2, 24, BF16, 128, 0, 4),
            ("tune-off-f32",    12, 2, 24, F32,  128, 0, 4),
            ("ld-odd",          12, 2, 24, BF16, 128, 1, 3),
            ("d64",             6,  2, 24, BF16, 64,  1, 4),
            ("d64-f32",         6,  2, 24, F32,  64,  1, 4),
            ("d16",             6,  2, 7,  BF16, 16,  1, 4),
            ("d16-f32",         6,  2, 7,  F32,  16,  1, 4)]
    for key, heads, kvh, R, dtype, d, tune, pad_q in rows:
        st = kernel_stride(dtype, d)
        counts = {1: [2 * st + 1], 3: [st, 1, st + 1], 7: [st + 1, 1, 2 * st, st - 1, 3 * st + 2, st, 2 * st + 1], 24: stride_counts(st)}[R]
        if d == 16:      # 16 dimensions cannot carry the edges of three strides: one stride and its neighbours
            counts = [st + 1, 1, st, st - 1, 2, st + 2, 5]
        for kind in ("plain", "planted"):
            s[f"{key}-{kind}"] = functools.partial(Case, f"C {key} {kind}", f"attn_head<{_dt(dtype)}>", heads, kvh, [n - 1 for n in counts],
                                                   [(3 * r + 2) % 4 for r in range(R)], kind, stride_edges(st, d), d=d, dtype=dtype, pad_q=pad_q, attn_group=tune)
    return s


def _specs_d():
    s = {}
    st = kernel_stride(BF16, 128)
    c24, crows = [n - 1 for n in stride_counts(st)], [(5 * r + 1) % 3 for r in range(24)]
    c15 = [n - 1 for n in stride_counts(st)[:15]]
    st64, st32 = kernel_stride(BF16, 64), kernel_stride(BF16, 32)
    c64 = [n - 1 for n in stride_counts(st64)]
    c32 = [n - 1 for n in (st32 + 1, 1, 2 * st32, st32 - 1, 2 * st32 + 1, st32, 3, 2 * st32 - 1) * 3]
    rows = {
        "vt-R15":      dict(route="attn_group<bf16,nq6,g16>", lens=c15, crows=crows[:15], vt=True, s_max=128),
        "vt-smax-odd": dict(route="attn_group<bf16,nq6,g16>", lens=c24, crows=crows, vt=True, s_max=max(c24) + 4),
        "vt-d64":      dict(route="attn_group<bf16,nq6,g0>", lens=c64, crows=crows, vt=True, d=64, s_max=224, st=st64),
        "vt-ldo-odd":  dict(route="attn_group<bf16,nq6,g16>", lens=c24, crows=crows, vt=True, s_max=128, pad_o=3),
        # bf16 head_dim 32: G = 4 lanes per key, ng = 4 * 16 = 64 key groups, NQ * ng = 384 > 256 threads: the per-head kernel
        "nq-ng-384":   dict(route="attn_head<bf16>", lens=c32, crows=crows, d=32, st=st32),
    }
    for key, a in rows.items():
        a = dict(a)
        route, lens, cr, stride = a.pop("route"), a.pop("lens"), a.pop("crows"), a.pop("st", st)
        for kind in ("plain", "planted"):
            s[f"{key}-{kind}"] = functools.partial(Case, f"D {key} {kind}", route, 12, 2, lens, cr, kind, stride_edges(stride, a.get("d", 128)), **a)
    return s


SPECS = {"A": _specs_a(), "B": _specs_b(), "C": _specs_c(), "D": _specs_d()}


@functools.lru_cache(maxsize=None)
def case_of(group, key):
    """every case is built once per session: the planted-cost check and the parity test share it and its reference"""
    return SPECS[group][key]()


ALL_KEYS = [(g, k) for g in SPECS for k in SPECS[g]]


@pytest.mark.parametrize("group", list(SPECS))
def test_planted_edges_carry_weight(group):
    """CPU only: in every planted case of the file, zeroing or doubling the weight of any one planted key in the fp64 reference moves its
    (row, head) by at least EDGE_COST - the inputs, not the kernel, keep that condition.  (Peaky cases are there for the running maximum: with
    scores of std 6 a chance key may outweigh the planted ones, so they carry no such claim.)"""
    worst = float("inf")
    for key in SPECS[group]:
        c = case_of(group, key)
        if c.kind != "planted":
            continue
        cost = c.edge_cost()
        worst = min(worst, cost)
        assert cost >= EDGE_COST, f"{c.name}: a planted edge moves its (row, head) by {cost:.3e} only (EDGE_COST {EDGE_COST:g})"
    print(f"{group}: the weakest planted edge of any case costs {worst:.3e}")


ALL_ROUTES = (["attn_prefill_mfma", "attn_head<bf16>", "attn_head<f32>"]
              + [f"attn_group<{t},nq{n},g{g}>" for t, gs in (("bf16", (16, 0)), ("f32", (32, 0))) for g in gs for n in (2, 6, 7)])


def _route(L, l, c, qkv_ptr, out_ptr, k_ptr, v_ptr, vt_ptr):
    kv = L.KV(k_ptr, v_ptr, L.VV_BF16 if c.dtype == BF16 else L.VV_F32, 2, c.n_rows, c.kvh, c.s_max, c.d, vt_ptr)
    name = C.create_string_buffer(64)
    l.vv_tune(b"attn_group", c.attn_group)
    try:
        L.check(l.vv_attn_route(qkv_ptr, c.ld_qkv, c.R, c.heads, C.byref(kv), out_ptr, c.ldo, name, 64), "vv_attn_route")
    finally:
        l.vv_tune(b"attn_group", 1)
    return name.value.decode()


def test_every_kernel_is_named_by_a_parity_case():
    """CPU only (vv_attn_route launches nothing and follows no pointer): every parity case takes the kernel it says it tests, and together the
    cases name the matrix-core kernel, all 12 attn_group instantiations and both attn_head ones.  The pointers are stand-ins with the
    alignment of a device allocation; the parity tests ask again with the real ones."""
    from vibevoice_rocm_amd import _lib as L
    l = L.load()
    seen = set()
    for group, key in ALL_KEYS:
        c = case_of(group, key)
        got = _route(L, l, c, 0x10000, 0x20000, 0x30000, 0x40000, 0x50000 if c.vt is not None else None)
        assert got == c.route, f"{c.name}: takes {got}, meant to test {c.route}"
        seen.add(got)
    assert seen == set(ALL_ROUTES), f"not reached: {sorted(set(ALL_ROUTES) - seen)}; unexpected: {sorted(seen - set(ALL_ROUTES))}"


def test_route_refuses_what_vv_attn_refuses():
    """CPU only: arguments vv_attn refuses before any launch get the same return code and the same error text from vv_attn_route - both take
    them from the one decision function.  The pointers are stand-ins that a refused call never follows."""
    from vibevoice_rocm_amd import _lib as L
    l = L.load()
    refused = {"fp8 cache": dict(kvdt=L.VV_FP8), "heads no multiple of kv_heads": dict(heads=13), "no rows": dict(R=0),
               "head_dim 24 on a bf16 cache": dict(d=24), "head_dim 1024 on an fp32 cache": dict(kvdt=L.VV_F32, d=1024)}
    for what, a in refused.items():
        kv = L.KV(0x30000, 0x40000, a.get("kvdt", L.VV_BF16), 2, 3, 2, 96, a.get("d", 128), None)
        R, heads = a.get("R", 24), a.get("heads", 12)
        name = C.create_string_buffer(64)
        rc_route = l.vv_attn_route(0x10000, 2052, R, heads, C.byref(kv), 0x20000, 1540, name, 64)
        err_route = l.vv_last_error().decode()
        rc_attn = l.vv_attn(0x10000, 2052, R, heads, C.byref(kv), 1, 0x60000, None, 0x20000, 1540, None)
        err_attn = l.vv_last_error().decode()
        assert rc_route != 0 and rc_route == rc_attn and err_route == err_attn and err_route, f"{what}: route {rc_route} '{err_route}', vv_attn {rc_attn} '{err_attn}'"
        assert name.value == b"", f"{what}: a refused call is given no kernel name"


# ---------------------------------------------------------------------------------------------------------------
# running and judging one call
# ---------------------------------------------------------------------------------------------------------------
def _attn(c):
    """the case's call on fresh device copies; returns out[R, ldo] on the CPU"""
    L, l = _lib()
    k, v, qkv = c.k.cuda(), c.v.cuda(), c.qkv.cuda()
    vt = c.vt.cuda() if c.vt is not None else None
    lens = torch.tensor(c.lens, dtype=torch.int32).cuda()
    crows = torch.tensor(c.crows, dtype=torch.int32).cuda() if c.crows is not None else None
    out = _sentinel((c.R, c.ldo)).cuda()
    got = _route(L, l, c, qkv.data_ptr(), out.data_ptr(), k.data_ptr(), v.data_ptr(), vt.data_ptr() if vt is not None else None)
    assert got == c.route, f"{c.name}: takes {got}, meant to test {c.route}"
    kv = L.KV(k.data_ptr(), v.data_ptr(), L.VV_BF16 if c.dtype == BF16 else L.VV_F32, 2, c.n_rows, c.kvh, c.s_max, c.d, vt.data_ptr() if vt is not None else None)
    l.vv_tune(b"attn_group", c.attn_group)
    try:
        L.check(l.vv_attn(qkv.data_ptr(), c.ld_qkv, c.R, c.heads, C.byref(kv), 1, lens.data_ptr(), crows.data_ptr() if crows is not None else None,
                          out.data_ptr(), c.ldo, None), "vv_attn")
        torch.cuda.synchronize()
    finally:
        l.vv_tune(b"attn_group", 1)
    for name, before, after in (("qkv", c.qkv, qkv), ("k", c.k, k), ("v", c.v, v)) + ((("vt", c.vt, vt),) if vt is not None else ()):
        assert torch.equal(_bits(before), _bits(after.cpu())), f"{c.name}: vv_attn changed {name}"
    return out.cpu()


def _per_head(o, want):
    return (o - want).pow(2).mean(-1).sqrt() / (want.pow(2).mean(-1).sqrt() + 1e-30)


def _judge(c, out, tag=None):
    """finite everywhere, pad columns untouched, and the bars of the case's kernel"""
    tag = tag or c.name
    R, heads, d = c.R, c.heads, c.d
    assert torch.equal(out[:, heads * d:].contiguous().view(torch.int32), torch.full((R, c.ldo - heads * d), SENT32, dtype=torch.int32)), f"{tag}: pad columns of out changed"
    o = out[:, : heads * d]
    assert bool(torch.isfinite(o).all()), f"{tag}: non-finite output"
    o = o.double().view(R, heads, d)
    want = c.ref()
    e = rel_rms(o.numpy(), want.numpy(), f"{tag}: whole call vs fp64")
    if c.route == "attn_prefill_mfma":
        wc = ref_prompt_contract(c.q, c.k[1], c.v[1], c.lens, c.crows, heads)
        ph = _per_head(o, wc)
        r_w, h_w = divmod(int(ph.argmax()), heads)
        eh = rel_rms(o[r_w, h_w].numpy(), wc[r_w, h_w].numpy(), f"{tag}: worst (row, head) = ({r_w}, {h_w}) vs the contract reference, {c.lens[r_w] + 1} keys")
        print(f"{tag}: global vs fp64 {e:.3e}  worst (row {r_w}, head {h_w}, {c.lens[r_w] + 1} keys) vs contract {eh:.3e}  [worst head vs fp64 {float(_per_head(o, want).max()):.3e}]")
        assert eh < MFMA_HEAD_BAR, f"{tag}: (row {r_w}, head {h_w}) with {c.lens[r_w] + 1} keys: rel RMS {eh:.3e} vs the contract reference (bar {MFMA_HEAD_BAR:g})"
        if c.kind != "peaky":
            assert e < MFMA_GLOBAL_BAR, f"{tag}: global rel RMS {e:.3e} vs fp64 (bar {MFMA_GLOBAL_BAR:g})"
    else:
        ph = _per_head(o, want)
        r_w, h_w = divmod(int(ph.argmax()), heads)
        eh = rel_rms(o[r_w, h_w].numpy(), want[r_w, h_w].numpy(), f"{tag}: worst (row, head) = ({r_w}, {h_w}), {c.lens[r_w] + 1} keys")
        print(f"{tag}: global {e:.3e}  worst (row {r_w}, head {h_w}, {c.lens[r_w] + 1} keys) {eh:.3e}")
        assert e < GLOBAL_BAR, f"{tag}: global rel RMS {e:.3e} (bar {GLOBAL_BAR:g})"
        assert eh < HEAD_BAR, f"{tag}: (row {r_w}, head {h_w}) with {c.lens[r_w] + 1} keys: rel RMS {eh:.3e} (bar {HEAD_BAR:g})"
    return e, eh


@pytest.mark.parametrize("key", list(SPECS["A"]))
def test_matrix_core_kernel_vs_fp64(key):
    """A.  attn_prefill_kernel: one wave per (32-query tile, q head), Q and P rounded to bf16 for the matrix cores.  Judged per (row, head)
    against the contract reference and per call against pure fp64 (module docstring)."""
    _need_gpu()
    c = case_of("A", key)
    _judge(c, _attn(c))


@pytest.mark.parametrize("key", list(SPECS["B"]))
def test_grouped_kernel_vs_fp64(key):
    """B.  attn_group_kernel<KT, EPL, NQ, GT>, reached with vt = NULL: one block per (row, KV head), keys two strides ahead of the arithmetic
    (stride = 4 * (64 / G) keys), clamped loads behind the row's last key."""
    _need_gpu()
    c = case_of("B", key)
    _judge(c, _attn(c))


@pytest.mark.parametrize("key", list(SPECS["C"]))
def test_per_head_kernel_vs_fp64(key):
    """C.  attn_kernel<KT, EPL>: one block per (row, q head), 4 * KPW keys per block step."""
    _need_gpu()
    c = case_of("C", key)
    _judge(c, _attn(c))


@pytest.mark.parametrize("key", list(SPECS["D"]))
def test_route_fallbacks_vs_fp64(key):
    """D.  Calls the matrix-core kernel (vt set) or the grouped kernel refuses: the route names the fall-back and the fall-back is right."""
    _need_gpu()
    c = case_of("D", key)
    _judge(c, _attn(c))


# ---------------------------------------------------------------------------------------------------------------
# E. vv_rope_store
# ---------------------------------------------------------------------------------------------------------------
E_POS = [0, 30, 31, 32, 33, 63, 64, 95]
E_SMAX = 96


def _rope_store(L, l, qkv, ld, heads, kv, lens_d, crows_d, inv_freq_d, d):
    R = qkv.shape[0]
    rope = torch.empty(R, d // 2, 2, device="cuda")
    L.check(l.vv_rope_table(lens_d.data_ptr(), inv_freq_d.data_ptr(), R, d, rope.data_ptr(), None), "vv_rope_table")
    L.check(l.vv_rope_store(qkv.data_ptr(), ld, R, heads, C.byref(kv), 1, rope.data_ptr(), lens_d.data_ptr(), crows_d.data_ptr() if crows_d is not None else None, None),
            "vv_rope_store")


@pytest.mark.parametrize("with_vt", [True, False], ids=["vt", "no_vt"])
@pytest.mark.parametrize("dtype,d", [(BF16, 128), (BF16, 64), (F32, 128), (F32, 64)], ids=["bf16_d128", "bf16_d64", "f32_d128", "f32_d64"])
def test_rope_store_vs_fp64(dtype, d, with_vt):
    """E.  vv_rope_store on 8 rows at positions 0, 30 .. 33, 63, 64 and s_max - 1 = 95 (both sides of two v^T tile boundaries), layer 1 of 2, for
    12 / 2, 28 / 4 and 4 / 2 heads (the two thread-strided loops run below, at and above one pass of 256 threads) and cache_rows NULL, a
    permutation, and all rows writing one cache row.  The table comes from vv_rope_table.  q is rotated in place and the stored k matches the
    fp64 rotation (fp32 arithmetic on a table correct to a few ulp: K_F32_BAR; a bf16 cache adds one rounding: K_BF16_BAR); the k / v sections
    and the pad columns of qkv keep their bits; the stored v is v rounded to the cache dtype and the v^T buffer is vt_tiles of the v cache; every
    other byte of k, v and v^T - the other layer and the unaddressed row included - keeps the sentinel it was filled with."""
    _need_gpu()
    L, l = _lib()
    R, inv_freq = len(E_POS), _inv_freq(d)
    worst_q = worst_k = 0.0
    for heads, kvh in ((12, 2), (28, 4), (4, 2)):
        for mode, crows, n_rows in (("null", None, R + 1), ("perm", [5, 2, 7, 0, 3, 6, 1, 4], R + 1), ("one-row", [2] * R, 4)):
            tag = f"E {_dt(dtype)} d={d} {'vt' if with_vt else 'no vt'} {heads}/{kvh} cache_rows {mode}"
            g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
            nat = (heads + 2 * kvh) * d
            ld = nat + 4
            qkv0 = _sentinel((R, ld))
            qkv0[:, :nat] = torch.randn(R, nat, generator=g)
            shape = (2, n_rows, kvh, E_SMAX, d)
            k0, v0 = _sentinel(shape, dtype), _sentinel(shape, dtype)
            vt0 = _sentinel((2, n_rows, kvh, E_SMAX // 32, d, 32), dtype) if with_vt else None
            qkv, k, v = qkv0.cuda(), k0.cuda(), v0.cuda()
            vt = vt0.cuda() if with_vt else None
            kv = L.KV(k.data_ptr(), v.data_ptr(), L.VV_BF16 if dtype == BF16 else L.VV_F32, 2, n_rows, kvh, E_SMAX, d, vt.data_ptr() if with_vt else None)
            lens_d = torch.tensor(E_POS, dtype=torch.int32).cuda()
            crows_d = torch.tensor(crows, dtype=torch.int32).cuda() if crows is not None else None
            _rope_store(L, l, qkv, ld, heads, kv, lens_d, crows_d, inv_freq.cuda(), d)
            torch.cuda.synchronize()
            qkv2, k2, v2 = qkv.cpu(), k.cpu(), v.cpu()
            q_w, k_w, v_w = ref_rope_store_fp64(qkv0[:, :nat], E_POS, inv_freq, heads, kvh, d)
            # q in place; the rest of qkv bit-identical
            q_g = qkv2[:, : heads * d].double().view(R, heads, d)
            assert bool(torch.isfinite(q_g).all()), f"{tag}: non-finite q"
            eq = max(rel_rms(q_g.numpy(), q_w.numpy(), f"{tag}: q in place"), float(_per_head(q_g, q_w).max()))
            assert eq < K_F32_BAR, f"{tag}: rotated q rel RMS {eq:.3e}, whole call or worst (row, head) (bar {K_F32_BAR:.2e})"
            assert torch.equal(_bits(qkv2[:, heads * d:].contiguous()), _bits(qkv0[:, heads * d:].contiguous())), f"{tag}: k / v sections or pad columns of qkv changed"
            # the addressed slots
            named = list(range(R)) if crows is None else crows
            exp_k, exp_v = k0.clone(), v0.clone()
            k_g = torch.stack([k2[1, named[r], :, E_POS[r]] for r in range(R)]).double()
            assert bool(torch.isfinite(k_g).all()), f"{tag}: non-finite stored k"
            ek = max(rel_rms(k_g.numpy(), k_w.numpy(), f"{tag}: stored k"), float(_per_head(k_g, k_w).max()))
            assert ek < (K_BF16_BAR if dtype == BF16 else K_F32_BAR), f"{tag}: stored k rel RMS {ek:.3e}, whole call or worst (row, KV head)"
            for r in range(R):
                exp_k[1, named[r], :, E_POS[r]] = k2[1, named[r], :, E_POS[r]]
                exp_v[1, named[r], :, E_POS[r]] = v_w[r].float().to(dtype)
            assert torch.equal(_bits(exp_v), _bits(v2)), f"{tag}: v cache is not (v rounded to the cache dtype at the addressed slots, untouched elsewhere)"
            assert torch.equal(_bits(exp_k), _bits(k2)), f"{tag}: k cache changed outside the addressed slots"
            if with_vt:
                assert torch.equal(_bits(vt_tiles(exp_v)), _bits(vt.cpu())), f"{tag}: v^T is not the 32-key-tiled transpose of the v cache"
            worst_q, worst_k = max(worst_q, eq), max(worst_k, ek)
    print(f"E {_dt(dtype)} d={d} {'vt' if with_vt else 'no vt'}: q in place {worst_q:.3e}  stored k {worst_k:.3e}  (largest of whole call / worst head over 9 calls)")


# ---------------------------------------------------------------------------------------------------------------
# F. store then attend, chunked
# ---------------------------------------------------------------------------------------------------------------
def test_store_then_attend_one_call_and_two_chunks():
    """F.  vv_rope_table -> vv_rope_store -> vv_attn on a bf16 cache with v^T for 77 prompt rows of cache row 1 (12 / 2 heads, layer 1 of 2,
    s_max 96), as one call and as two chunks (40 rows at 0, 37 rows at 40: the chunk edge lies inside the second 32-key tile).  Both are judged
    like group A against fp64 causal attention over the rotated keys as stored (the cache and the rotated q read back and widened).  A query's
    result depends on its own accumulator column and on the key tiles in their fixed order only, never on which rows share its wave, so the
    two runs must agree bit for bit - outputs and caches."""
    _need_gpu()
    L, l = _lib()
    heads, kvh, d, R, s_max, n_rows = 12, 2, 128, 77, 96, 3
    nat = (heads + 2 * kvh) * d
    ld, ldo = nat + 4, heads * d + 4
    g = torch.Generator().manual_seed(77)
    qkv0 = _sentinel((R, ld))
    qkv0[:, :nat] = torch.randn(R, nat, generator=g)
    inv_freq_d = _inv_freq(d).cuda()

    def run(chunks):
        shape = (2, n_rows, kvh, s_max, d)
        k, v, vt = (torch.full(shape, float("nan"), dtype=BF16).cuda() for _ in range(3))
        kv = L.KV(k.data_ptr(), v.data_ptr(), L.VV_BF16, 2, n_rows, kvh, s_max, d, vt.data_ptr())
        qkv, out = qkv0.cuda(), _sentinel((R, ldo)).cuda()
        for a, b in chunks:
            lens_d = torch.arange(a, b, dtype=torch.int32).cuda()
            crows_d = torch.ones(b - a, dtype=torch.int32).cuda()
            name = C.create_string_buffer(64)
            L.check(l.vv_attn_route(qkv[a:].data_ptr(), ld, b - a, heads, C.byref(kv), out[a:].data_ptr(), ldo, name, 64), "vv_attn_route")
            assert name.value.decode() == "attn_prefill_mfma"
            _rope_store(L, l, qkv[a:b], ld, heads, kv, lens_d, crows_d, inv_freq_d, d)
            L.check(l.vv_attn(qkv[a:].data_ptr(), ld, b - a, heads, C.byref(kv), 1, lens_d.data_ptr(), crows_d.data_ptr(), out[a:].data_ptr(), ldo, None), "vv_attn")
            torch.cuda.synchronize()
        return qkv.cpu(), out.cpu(), k.cpu(), v.cpu(), vt.cpu()

    one, two = run([(0, R)]), run([(0, 40), (40, R)])
    for tag, (qkv2, out, k2, v2, vt2) in (("F one call", one), ("F two chunks", two)):
        assert torch.equal(out[:, heads * d:].contiguous().view(torch.int32), torch.full((R, 4), SENT32, dtype=torch.int32)), f"{tag}: pad columns of out changed"
        assert torch.equal(_bits(vt_tiles(v2)).reshape(-1), _bits(vt2).reshape(-1)), f"{tag}: v^T is not the 32-key-tiled transpose of the v cache"
        o = out[:, : heads * d]
        assert bool(torch.isfinite(o).all()), f"{tag}: non-finite output"
        o = o.double().view(R, heads, d)
        q = qkv2[:, : heads * d].view(R, heads, d)
        lens, crows = list(range(R)), [1] * R
        want = ref_prompt_fp64(q, k2[1], v2[1], lens, crows, heads)
        wc = ref_prompt_contract(q, k2[1], v2[1], lens, crows, heads)
        e = rel_rms(o.numpy(), want.numpy(), f"{tag}: whole call vs fp64")
        ph = _per_head(o, wc)
        r_w, h_w = divmod(int(ph.argmax()), heads)
        eh = rel_rms(o[r_w, h_w].numpy(), wc[r_w, h_w].numpy(), f"{tag}: worst (row, head) = ({r_w}, {h_w}) vs the contract reference")
        print(f"{tag}: global vs fp64 {e:.3e}  worst (row {r_w}, head {h_w}) vs contract {eh:.3e}")
        assert eh < MFMA_HEAD_BAR and e < MFMA_GLOBAL_BAR, f"{tag}: worst (row, head) {eh:.3e} vs contract, global {e:.3e} vs fp64"
    for name, a, b in zip(("qkv", "out", "k", "v", "vt"), one, two):
        same = torch.equal(_bits(a), _bits(b))
        print(f"F one call vs two chunks: {name} {'bit-identical' if same else 'DIFFERS'}")
        assert same, f"F: {name} of the two-chunk run differs from the one-call run"
