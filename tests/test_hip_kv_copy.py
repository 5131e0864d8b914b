"""vv_kv_copy (include/vv_hip.h) straight through the C ABI on the GPU: slots [0, len) of one cache row into a row of another cache - k and v
bit for bit, the destination's tile-major vt rebuilt from v, and nothing else touched.  The destination starts as the bf16 NaN pattern
0xFFFF (fp32: 0xFFFFFFFF), so a write outside the copied slots - or a slot left unwritten inside them - shows as a changed / unchanged word.

Shapes are the smallest that reach every index: 2 layers; 2 and 4 KV heads at head_dim 128 (bf16, with vt); the tiny preset's head_dim 16 in
fp32 without vt; len 7 / 32 / 45 / 64 = below a 32-key tile, exactly one, one and a partial one, exactly two; a one-row source with s_max 64
into row 1 of a 2-row and row 2 of a 4-row destination with s_max 128."""
import ctypes as C

import pytest
import torch

from conftest import vt_tiles

pytestmark = pytest.mark.gpu

LAYERS, S_SRC, S_DST = 2, 64, 128


def _lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    return L, L.load()


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _pattern(shape, dtype):
    """every word all ones: a NaN in bf16 and in fp32"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    _bits(t).fill_(-1)
    return t


def _cache(L, rows, kvh, s_max, d, dtype, with_vt, g=None):
    """(vv_kv, k, v, vt): random values when a generator is given, the NaN pattern otherwise"""
    shape = (LAYERS, rows, kvh, s_max, d)
    if g is not None:
        k = torch.randn(shape, generator=g).to(dtype).cuda()
        v = torch.randn(shape, generator=g).to(dtype).cuda()
        vt = vt_tiles(v) if with_vt else None
    else:
        k, v = _pattern(shape, dtype), _pattern(shape, dtype)
        vt = _pattern((LAYERS, rows, kvh, s_max // 32, d, 32), dtype) if with_vt else None
    kv = L.KV(k.data_ptr(), v.data_ptr(), L.VV_F32 if dtype == torch.float32 else L.VV_BF16, LAYERS, rows, kvh, s_max, d, L.ptr(vt), None, None)
    return kv, k, v, vt


def _check_row(k, v, vt, row, sk, sv, src_row, n):
    """destination (k, v, vt) after a copy of n slots of source row src_row into `row`: the slots bit for bit, everything else the pattern"""
    want_k, want_v = _pattern(k.shape, k.dtype), _pattern(v.shape, v.dtype)
    want_k[:, row, :, :n] = sk[:, src_row, :, :n]
    want_v[:, row, :, :n] = sv[:, src_row, :, :n]
    assert torch.equal(_bits(k), _bits(want_k)), "k: copied slots bit-identical, every other element untouched"
    assert torch.equal(_bits(v), _bits(want_v)), "v: copied slots bit-identical, every other element untouched"
    if vt is not None:
        want_vt = vt_tiles(want_v)          # columns >= n and the other rows: the pattern again
        assert torch.equal(_bits(vt), _bits(want_vt)), "vt: conftest.vt_tiles of the copied v for columns < len, untouched elsewhere"


@pytest.mark.parametrize("src_vt", [False, True])
@pytest.mark.parametrize("rows,dst_row", [(2, 1), (4, 2)])
@pytest.mark.parametrize("n", [7, 32, 45, 64])
@pytest.mark.parametrize("kvh", [2, 4])
def test_kv_copy_bf16_with_vt(kvh, n, rows, dst_row, src_vt):
    L, lib = _lib()
    g = torch.Generator().manual_seed(100 * kvh + n)
    src, sk, sv, _ = _cache(L, 1, kvh, S_SRC, 128, torch.bfloat16, src_vt, g)
    dst, k, v, vt = _cache(L, rows, kvh, S_DST, 128, torch.bfloat16, True)
    L.check(lib.vv_kv_copy(C.byref(src), 0, C.byref(dst), dst_row, n, None), "vv_kv_copy")
    torch.cuda.synchronize()
    _check_row(k, v, vt, dst_row, sk, sv, 0, n)


@pytest.mark.parametrize("n", [7, 32, 45, 64])
def test_kv_copy_fp32_without_vt(n, tiny_cfg):
    L, lib = _lib()
    d = tiny_cfg.head_dim
    g = torch.Generator().manual_seed(n)
    src, sk, sv, _ = _cache(L, 1, tiny_cfg.kv_heads, S_SRC, d, torch.float32, False, g)
    dst, k, v, _ = _cache(L, 2, tiny_cfg.kv_heads, S_DST, d, torch.float32, False)
    L.check(lib.vv_kv_copy(C.byref(src), 0, C.byref(dst), 1, n, None), "vv_kv_copy")
    torch.cuda.synchronize()
    _check_row(k, v, None, 1, sk, sv, 0, n)


def test_kv_copy_round_trip_store_cache_store():
    """store -> row 2 of a 4-row cache with vt -> a second store: the second store equals the first in its 45 slots and is untouched beyond"""
    L, lib = _lib()
    n = 45
    g = torch.Generator().manual_seed(3)
    s1, k1, v1, _ = _cache(L, 1, 2, S_SRC, 128, torch.bfloat16, False, g)
    cache, ck, cv, cvt = _cache(L, 4, 2, S_DST, 128, torch.bfloat16, True)
    s2, k2, v2, _ = _cache(L, 1, 2, S_SRC, 128, torch.bfloat16, False)
    L.check(lib.vv_kv_copy(C.byref(s1), 0, C.byref(cache), 2, n, None), "store -> cache")
    L.check(lib.vv_kv_copy(C.byref(cache), 2, C.byref(s2), 0, n, None), "cache -> store")
    torch.cuda.synchronize()
    _check_row(ck, cv, cvt, 2, k1, v1, 0, n)
    _check_row(k2, v2, None, 0, k1, v1, 0, n)


def test_kv_copy_len_zero_launches_nothing():
    L, lib = _lib()
    src, sk, sv, _ = _cache(L, 1, 2, S_SRC, 128, torch.bfloat16, False, torch.Generator().manual_seed(1))
    dst, k, v, vt = _cache(L, 2, 2, S_DST, 128, torch.bfloat16, True)
    assert lib.vv_kv_copy(C.byref(src), 0, C.byref(dst), 1, 0, None) == 0
    torch.cuda.synchronize()
    _check_row(k, v, vt, 1, sk, sv, 0, 0)


def test_kv_copy_refusals():
    """status only: nothing is launched, the destination keeps its pattern"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(2)
    src, sk, sv, _ = _cache(L, 1, 2, S_SRC, 128, torch.bfloat16, False, g)
    dst, k, v, vt = _cache(L, 2, 2, S_DST, 128, torch.bfloat16, True)
    VV_E_ARG, VV_E_UNSUPPORTED = -1, -3

    def variant(base, **kw):
        kv = L.KV()
        C.memmove(C.byref(kv), C.byref(base), C.sizeof(kv))
        for name, val in kw.items():
            setattr(kv, name, val)
        return kv

    assert lib.vv_kv_copy(C.byref(variant(src, kvdt=L.VV_FP8)), 0, C.byref(dst), 1, 7, None) == VV_E_UNSUPPORTED
    assert b"fp8" in lib.vv_last_error()
    assert lib.vv_kv_copy(C.byref(src), 0, C.byref(variant(dst, kvdt=L.VV_FP8)), 1, 7, None) == VV_E_UNSUPPORTED
    assert lib.vv_kv_copy(C.byref(variant(src, kv_heads=4)), 0, C.byref(dst), 1, 7, None) == VV_E_ARG          # mismatched kv_heads
    assert lib.vv_kv_copy(C.byref(src), 0, C.byref(dst), 1, S_SRC + 1, None) == VV_E_ARG                        # len > src s_max
    assert lib.vv_kv_copy(C.byref(dst), 0, C.byref(src), 0, S_SRC + 1, None) == VV_E_ARG                        # len > dst s_max
    assert lib.vv_kv_copy(C.byref(src), 1, C.byref(dst), 1, 7, None) == VV_E_ARG                                # source row out of range
    assert lib.vv_kv_copy(C.byref(src), 0, C.byref(dst), 2, 7, None) == VV_E_ARG                                # destination row out of range
    assert lib.vv_kv_copy(C.byref(variant(src, kvdt=L.VV_F32)), 0, C.byref(dst), 1, 7, None) == VV_E_ARG        # dtypes differ
    torch.cuda.synchronize()
    _check_row(k, v, vt, 1, sk, sv, 0, 0)
