"""The seeded token draws (vv_token_draws and the _rows step tails, include/vv_hip.h) restated in numpy on top of tests/philox_ref.py, as the
tests' reference: the Philox counter layout of the token domain, the float32 uniforms exactly as the kernel forms them, q = -ln u evaluated in
float64 from those float32 uniforms (with the clamp at u == 1), and the sampler's choice - warpers, softmax, argmax p / q - in float64 with the
final division in float32, as vv_sampler states it.  Test infrastructure only (tests/test_host_token_seed.py, tests/test_hip_token_seed.py): no
product path imports it."""
import numpy as np

import philox_ref as P

TINY = float(np.float32(2.0 ** -126))        # the smallest positive normal float: q where -ln u is 0 (u == 1)
GREEDY = (0.0, 0, 1.0)

# (seed, position, element): the Philox word of this draw is >= 2^32 - 128, so it converts to 2^32 in float32 and u == 1 exactly - the one case
# in ~2^25 words in which -logf(u) is 0 and the clamp decides.  Found by find_clamp_triple() below (tests/test_host_token_seed.py re-derives it).
CLAMP_TRIPLE = (0, 5937807, 7)


def counters(pos, elem):
    """the Philox counter words (quad, position, 0, 1) of element `elem` at draw index `pos`, and the output word the element is"""
    elem = np.asarray(elem, dtype=np.uint64)
    return (elem // np.uint64(4), np.asarray(pos, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF), 0, 1), elem % np.uint64(4)


def words(seed, pos, nv=8):
    """uint64 [..., nv]: the 32-bit Philox words behind q[0 .. nv) of (seed, pos); seed and pos broadcast against each other"""
    seed = np.asarray(seed, dtype=np.uint64)
    pos = np.asarray(pos, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    seed, pos = np.broadcast_arrays(seed, pos)
    key = (seed & np.uint64(0xFFFFFFFF), seed >> np.uint64(32))
    quads = [np.stack(P.philox4x32_10((j, pos, 0, 1), key), axis=-1) for j in range((nv + 3) // 4)]
    return np.concatenate(quads, axis=-1)[..., :nv]


def uniforms(seed, pos, nv=8):
    """float32 [..., nv]: u = (float) x * 2^-32 + 2^-33 in (0, 1]"""
    return P.uniform(words(seed, pos, nv))


def q_from_u(u):
    """float64: -ln u of float32 uniforms, TINY where that is 0"""
    q = -np.log(np.asarray(u, dtype=np.float32).astype(np.float64))
    return np.where(q > 0, q, TINY)


def draws(seed, pos, nv=8):
    """float64 [..., nv]: the exponential draws q of (seed, pos), evaluated in float64 from the float32 uniforms"""
    return q_from_u(uniforms(seed, pos, nv))


def choice(logits, q, row, ids=None):
    """(index, margin) the sampler picks for float32 `logits` [nv], draws `q` [nv] and the row (temperature, top_k, top_p).  A greedy row
    (temperature <= 0) takes the first maximum, the smallest id on ties (`ids`, default the index order); its margin is inf for a unique maximum
    and 1 on a tie.  Otherwise: vv_sampler's steps 1-5, margin = best / second-best of the float32 p / q."""
    l = np.asarray(logits, dtype=np.float32).astype(np.float64)
    nv = l.size
    t, k, p = float(np.float32(row[0])), int(row[1]), float(np.float32(row[2]))
    if not t > 0:
        ids = np.arange(nv) if ids is None else np.asarray(ids)
        best = 0
        for i in range(1, nv):
            if l[i] > l[best] or (l[i] == l[best] and ids[i] < ids[best]):
                best = i
        others = np.delete(l, best)
        return best, (float("inf") if others.size == 0 or l[best] > others.max() else 1.0)
    z = l / t
    keep = np.ones(nv, dtype=bool)
    order = np.argsort(z, kind="stable")                       # ascending, stable: the kernel's ranks
    if 0 < k < nv:
        kth = z[order[nv - k]]
        keep &= ~(z < kth)
    e = np.where(keep, np.exp(z - z.max()), 0.0)
    if p < 1.0:
        S = e[order].sum()
        cum = np.cumsum(e[order] / S)
        remove = cum <= (1.0 - p)
        remove[-1] = False
        keep[order[remove]] = False
        e = np.where(keep, e, 0.0)
    pr = (e / e.sum()).astype(np.float32)
    v = pr / np.asarray(q, dtype=np.float32)
    best = int(np.argmax(v))
    second = np.delete(v, best).max() if nv > 1 else 0.0
    return best, (float("inf") if second == 0 else float(v[best]) / float(second))


def token_stream(logits_of, seed, row, positions, ids=None):
    """the indices the sampler picks at `positions` for logits_of(position) -> float32 [nv]"""
    out = []
    for p in positions:
        l = logits_of(p)
        out.append(choice(l, draws(seed, p, len(l)).astype(np.float32), row, ids)[0])
    return out


def find_clamp_triple(seed=0, block=1 << 20, first_block=0, max_blocks=256):
    """the first (seed, position, element) in ascending position whose word is >= 2^32 - 128 (vectorised: `block` positions x 8 words at a time,
    from position first_block * block on)"""
    for b in range(first_block, first_block + max_blocks):
        pos = np.arange(b * block, (b + 1) * block, dtype=np.int64)
        w = words(seed, pos, 8)
        hit = np.argwhere(w >= np.uint64(2 ** 32 - 128))
        if hit.size:
            i, e = hit[0]
            return (int(seed), int(pos[i]), int(e))
    return None
