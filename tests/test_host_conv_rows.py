"""Host side of the row-batched conv tails (batched_conv_rows), CPU only: the six entry points load, the keyword's ValueErrors fire before
any weight is touched, the drivers build today's row-batch keys with the flag off (and keys of their own with it on), and the bookkeeping
object (rowbatch.ConvRowsBook) - who owes a back, which mask every call uploads - driven with scripted steps."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

from vibevoice_rocm_amd import _lib, modeling
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as Model
from vibevoice_rocm_amd.modeling import check_batched_conv_rows
from vibevoice_rocm_amd.rowbatch import ConvRowsBook

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["vv_conv_rows_ws_bytes", "vv_decoder_front_rows", "vv_decoder_forward_from", "vv_encoder_forward_until", "vv_encoder_back_rows",
           "vv_connector_pair_rows"]


def test_symbols_load_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.vv_abi_version() == 6
    hdr = open(os.path.join(ROOT, "include", "vv_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in SYMBOLS:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
        assert re.search(r"\b" + name + r"\s*\(", plain), name
    vp, i64 = C.c_void_p, C.c_int64
    nets = C.POINTER(C.POINTER(_lib.ConvNet))
    assert _lib.PROTOTYPES["vv_decoder_front_rows"] == (C.c_int, [nets, C.c_int, vp, vp, i64, C.c_float, C.c_float, vp, i64, vp, vp])
    assert _lib.PROTOTYPES["vv_encoder_back_rows"] == (C.c_int, [nets, C.c_int, vp, vp, i64, vp, i64, vp, vp])
    assert _lib.PROTOTYPES["vv_conv_rows_ws_bytes"][0] is C.c_size_t
    # plain arguments only: the struct mirrors are what they were
    assert lib.vv_sizeof(b"vv_convnet") == C.sizeof(_lib.ConvNet) and lib.vv_sizeof(b"vv_block") == C.sizeof(_lib.Block)


def test_refusals_without_a_device():
    """the argument checks come before anything touches the device: they answer on a machine without one"""
    lib = _lib.load()
    net = _lib.ConvNet()
    assert lib.vv_conv_rows_ws_bytes(None, 4, 1) == 0
    assert lib.vv_conv_rows_ws_bytes(C.byref(net), 1, 1) == 0 and lib.vv_conv_rows_ws_bytes(C.byref(net), 9, 1) == 0
    assert lib.vv_conv_rows_ws_bytes(C.byref(net), 4, 1) == 0          # an empty net is not covered
    assert lib.vv_decoder_front_rows(None, 4, None, None, 0, 1.0, 0.0, None, 0, None, None) == -1
    assert lib.vv_decoder_forward_from(C.byref(net), None, None, None, None) == -1
    assert lib.vv_encoder_forward_until(C.byref(net), None, 3200, None, None, None) == -1
    assert lib.vv_encoder_back_rows(None, 4, None, None, 0, None, 0, None, None) == -1


@pytest.mark.parametrize("kw", [dict(weight_quant="fp8"), dict(weight_quant="nf4"), dict(weight_quant="mxfp4"), dict(torch_dtype=torch.float32), dict()])
def test_value_errors_before_any_weight_is_touched(kw):
    """the state dict is empty: a KeyError would mean the check came too late.  The tiny preset's tokenizers have 2 filters, so the plain
    bf16 call is refused for its one-row stage's width"""
    with pytest.raises(ValueError, match="batched_conv_rows"):
        Model(VVConfig.preset("tiny"), {}, batched_conv_rows=True, **kw)
    a = dict(torch_dtype=torch.bfloat16, weight_quant=None)
    a.update(kw)
    if kw:
        with pytest.raises(ValueError, match="batched_conv_rows"):
            check_batched_conv_rows(True, a["torch_dtype"], a["weight_quant"], VVConfig.preset("1.5b"))
    assert check_batched_conv_rows(False, a["torch_dtype"], a["weight_quant"], VVConfig.preset("tiny")) is False      # off: nothing is checked


def test_accepted_on_the_shipped_presets():
    for name in ("1.5b", "7b"):
        assert check_batched_conv_rows(True, torch.bfloat16, None, VVConfig.preset(name)) is True
    with pytest.raises(ValueError, match="n_filters"):
        check_batched_conv_rows(True, torch.bfloat16, None, VVConfig.preset("mid"))


class _FakeBatch:
    """the stand-in of tests/test_host_rows16.py: RowBatch(lanes, stream=None) and nothing of the new mode"""
    made = []

    def __init__(self, lanes, stream=None):
        self.lanes, self.B = lanes, len(lanes)
        self.enabled = False
        _FakeBatch.made.append(self)

    def begin(self, *a, **k):
        pass

    def set_active(self, *a):
        pass


class _FakeBatchRows(_FakeBatch):
    def enable_conv_rows(self):
        self.enabled = True


def _fake_model(width, **extra):
    lanes = {}

    def lane(i):
        return lanes.setdefault(i, SimpleNamespace(i=i, sde=False, n_steps=10))
    m = SimpleNamespace(_lane=lane, _rowbatch={}, row_batch_width=width, **extra)
    m.engine = lane(0)
    m.engine.stream = None
    m._lanes = [m.engine]
    return m


@pytest.mark.parametrize("width, B, keys", [(4, 6, [(3, 0, "side"), (3, 3, "side")]), (8, 6, [(6, 0, "side")]), (4, 4, [(4, 0)])])
def test_flag_off_builds_todays_keys(monkeypatch, width, B, keys):
    from vibevoice_rocm_amd import rowbatch
    monkeypatch.setattr(rowbatch, "RowBatch", _FakeBatch)        # has no enable_conv_rows: calling it would raise
    monkeypatch.setattr(modeling, "_embed_prompt", lambda *a: None)
    m = _fake_model(width)                                       # a model without the attribute: read with getattr(..., False)
    d = modeling._RowDriver(m, B, 2.0, 1, 2)
    assert d.conv_rows is False
    d.begin([[0] * 5] * B, [None] * B, 4, [1, 2])
    assert list(m._rowbatch) == keys
    s = modeling._SessionDriver(_fake_model(4), 3, 1, 2, True)
    s.open(256, [1, 2])
    assert list(s.model._rowbatch) == [(3, 0, "session")]


def test_flag_on_gets_keys_of_its_own_and_enables_after_construction(monkeypatch):
    from vibevoice_rocm_amd import rowbatch
    monkeypatch.setattr(rowbatch, "RowBatch", _FakeBatchRows)
    monkeypatch.setattr(modeling, "_embed_prompt", lambda *a: None)
    m = _fake_model(4, batched_conv_rows=True)
    d = modeling._RowDriver(m, 6, 2.0, 1, 2)
    assert d.conv_rows is True
    d.begin([[0] * 5] * 6, [None] * 6, 4, [1, 2])
    assert list(m._rowbatch) == [(3, 0, "side", "conv_rows"), (3, 3, "side", "conv_rows")]
    assert all(rb.enabled for rb in m._rowbatch.values())
    # the per-call override switches it off on the same model: today's keys next to the others
    d2 = modeling._RowDriver(m, 6, 2.0, 1, 2)
    d2.conv_rows = False
    d2.begin([[0] * 5] * 6, [None] * 6, 4, [1, 2])
    assert list(m._rowbatch)[2:] == [(3, 0, "side"), (3, 3, "side")] and not any(m._rowbatch[k].enabled for k in list(m._rowbatch)[2:])
    s = modeling._SessionDriver(m, 3, 1, 2, True)                # a session inherits the model's value
    s.open(256, [1, 2])
    assert (3, 0, "session", "conv_rows") in m._rowbatch


# ---- the bookkeeping object, scripted ----------------------------------------------------------------------------------------------------

def test_book_two_speech_calls_in_a_step_one_back_over_the_union():
    bk = ConvRowsBook(4)
    assert bk.back() is None                                   # the first graph A of a batch: nobody owes anything
    assert bk.front([0, 2]) == [1, 0, 1, 0]                    # the speculated dialogues
    assert bk.front([3]) == [0, 0, 0, 1]                       # the rest, later in the step
    assert bk.owed == {0, 2, 3}
    assert bk.back() == [1, 0, 1, 1]                           # once, in front of the next graph A
    assert bk.back() is None and bk.owed == set()
    assert bk.log == [("front", (1, 0, 1, 0)), ("front", (0, 0, 0, 1)), ("back", (1, 0, 1, 1))]


def test_book_speculate_then_roll_back():
    bk = ConvRowsBook(3)
    assert bk.front([0, 1, 2]) == [1, 1, 1]
    bk.rollback(1)                                             # dialogue 1's token was not a diffusion token: its frame is undone, embed(1) writes its x rows
    assert bk.back() == [1, 0, 1]
    bk.front([1])
    bk.rollback(1)
    bk.rollback(1)                                             # twice is harmless
    assert bk.back() is None                                   # everybody rolled back: no back at all


def test_book_restart_and_a_step_where_nobody_diffuses():
    bk = ConvRowsBook(2)
    bk.front([0, 1])
    bk.restart()                                               # RowBatch.begin: a new batch on the same object
    assert bk.owed == set() and bk.back() is None
    assert bk.back() is None                                   # steps of text tokens: no front, no back, no mask uploaded
    assert [k for k, _ in bk.log] == ["front"]
    bk.front([1])
    assert bk.back() == [0, 1]


def test_book_refuses_what_cannot_be():
    bk = ConvRowsBook(2)
    with pytest.raises(ValueError):
        bk.front([2])
    with pytest.raises(ValueError):
        bk.front([])
    assert bk.owed == set() and bk.log == []
