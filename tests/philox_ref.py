"""The device noise generator (vv_noise_normal in include/vv_hip.h) restated in numpy, as the tests' reference: Philox4x32-10 in uint64
integer arithmetic, the uniforms in float32 exactly as the kernel forms them, the Box-Muller transform evaluated in float64 from those float32
uniforms.  Test infrastructure only (tests/test_host_device_noise.py, tests/test_hip_device_noise.py): no product path imports it."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # Weyl constants the key is bumped by
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two; broadcast against each other.  Returns the four uint64 arrays of 32-bit outputs."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in counter]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & _MASK for x in key)
    c = list(np.broadcast_arrays(*c, k0, k1)[:4])
    for r in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]          # 32 x 32 -> 64 bits: exact in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return c


def uniform(x):
    """u = (float) x * 2^-32 + 2^-33 in float32: the conversion rounds to nearest even, the product is exact, the sum rounds once; (0, 1]"""
    return (np.asarray(x, dtype=np.uint64).astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)).astype(np.float32)


def box_muller(u0, u1):
    """(r cos(2 pi u1), r sin(2 pi u1)), r = sqrt(-2 ln u0), in float64 from float32 uniforms"""
    u0, u1 = np.asarray(u0, dtype=np.float32).astype(np.float64), np.asarray(u1, dtype=np.float32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u0))
    return r * np.cos(2.0 * np.pi * u1), r * np.sin(2.0 * np.pi * u1)


def normal_quads(seed, frame, kind, quads):
    """float64 [len(quads), 4]: the normals of the given quads of the row (seed, frame, kind)"""
    seed = int(seed) & (2 ** 64 - 1)
    j = np.asarray(quads, dtype=np.uint64)
    x = philox4x32_10((j, int(frame) & 0xFFFFFFFF, int(kind), 0), (seed & 0xFFFFFFFF, seed >> 32))
    u = [uniform(v) for v in x]
    z0, z1 = box_muller(u[0], u[1])
    z2, z3 = box_muller(u[2], u[3])
    return np.stack([z0, z1, z2, z3], axis=-1)


def normal_row(seed, frame, kind, n):
    """float64 [n]: row `kind` (0: the initial latent, 1 + s: the variance noise of solver step s) of frame `frame` of the dialogue with `seed`"""
    return normal_quads(seed, frame, kind, np.arange((n + 3) // 4)).reshape(-1)[:n]
