"""Host side of wide row batches (row_batch_width), CPU only: the partition of B dialogues into row batches at both widths, the ValueErrors of
the keyword, and that the model's width reaches the two drivers that partition (modeling._RowDriver.begin, _SessionDriver.open)."""
from types import SimpleNamespace

import pytest
import torch

from vibevoice_rocm_amd import modeling
from vibevoice_rocm_amd.config import VVConfig
from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as Model
from vibevoice_rocm_amd.modeling import check_row_batch_width, row_partition

# what _RowDriver.begin built before the keyword existed: ceil(B / 4) balanced groups
WIDTH4 = {2: [2], 3: [3], 4: [4], 5: [3, 2], 6: [3, 3], 7: [4, 3], 8: [4, 4], 9: [3, 3, 3], 10: [4, 3, 3], 11: [4, 4, 3], 12: [4, 4, 4],
          13: [4, 3, 3, 3], 14: [4, 4, 3, 3], 15: [4, 4, 4, 3], 16: [4, 4, 4, 4]}
WIDTH8 = {2: [2], 3: [3], 4: [4], 5: [5], 6: [6], 7: [7], 8: [8], 9: [5, 4], 10: [5, 5], 11: [6, 5], 12: [6, 6], 13: [7, 6], 14: [7, 7],
          15: [8, 7], 16: [8, 8]}


@pytest.mark.parametrize("B", range(2, 17))
def test_partition(B):
    assert row_partition(B, 4) == WIDTH4[B] == row_partition(B)
    n_groups = -(-B // 4)
    assert WIDTH4[B] == [B // n_groups + (1 if g < B % n_groups else 0) for g in range(n_groups)]      # the expression the drivers held
    assert row_partition(B, 8) == WIDTH8[B]
    assert sum(WIDTH8[B]) == B and len(WIDTH8[B]) == -(-B // 8) and max(WIDTH8[B]) - min(WIDTH8[B]) <= 1


@pytest.mark.parametrize("width", [0, 2, 5, 16, "8", None, True, 8.5])
def test_other_widths_are_refused(width):
    with pytest.raises(ValueError, match="row_batch_width"):
        check_row_batch_width(width, torch.bfloat16, None, None)
    with pytest.raises(ValueError, match="row_batch_width"):
        Model(VVConfig.preset("tiny"), {}, row_batch_width=width)


@pytest.mark.parametrize("kw", [dict(weight_quant="fp8"), dict(weight_quant="nf4"), dict(weight_quant="mxfp4"), dict(torch_dtype=torch.float32),
                                dict(kv_cache_dtype="fp8")])
def test_width_8_needs_bf16_weights_and_cache(kw):
    """raised at construction, before any weight is touched (the state dict is empty)"""
    with pytest.raises(ValueError, match="row_batch_width=8"):
        Model(VVConfig.preset("tiny"), {}, row_batch_width=8, **kw)
    a = dict(torch_dtype=torch.bfloat16, weight_quant=None, kv_cache_dtype=None)
    a.update(kw)
    with pytest.raises(ValueError, match="row_batch_width=8"):
        check_row_batch_width(8, a["torch_dtype"], a["weight_quant"], a["kv_cache_dtype"])
    assert check_row_batch_width(4, a["torch_dtype"], a["weight_quant"], a["kv_cache_dtype"]) == 4      # the default width takes them all


def test_width_8_is_accepted_on_bf16():
    assert check_row_batch_width(8, torch.bfloat16, None, None) == 8 and check_row_batch_width(8, torch.bfloat16, None, "bf16") == 8


class _FakeBatch:
    made = []

    def __init__(self, lanes, stream=None):
        self.lanes, self.B = lanes, len(lanes)
        _FakeBatch.made.append(self)

    def begin(self, *a, **k):
        pass

    def set_active(self, *a):
        pass


def _fake_model(width):
    lanes = {}

    def lane(i):
        return lanes.setdefault(i, SimpleNamespace(i=i, sde=False, n_steps=10))
    m = SimpleNamespace(_lane=lane, _rowbatch={}, row_batch_width=width)
    m.engine = lane(0)
    m.engine.stream = None
    m._lanes = [m.engine]
    return m


@pytest.mark.parametrize("width, B, keys", [(4, 6, [(3, 0, "side"), (3, 3, "side")]), (8, 6, [(6, 0, "side")]), (8, 10, [(5, 0, "side"), (5, 5, "side")]),
                                            (8, 4, [(4, 0)]), (4, 4, [(4, 0)]), (8, 16, [(8, 0, "side"), (8, 8, "side")])])
def test_width_reaches_the_row_driver(monkeypatch, width, B, keys):
    from vibevoice_rocm_amd import rowbatch
    monkeypatch.setattr(rowbatch, "RowBatch", _FakeBatch)
    monkeypatch.setattr(modeling, "_embed_prompt", lambda *a: None)
    m = _fake_model(width)
    d = modeling._RowDriver(m, B, 2.0, 1, 2)
    assert d.width == width
    d.begin([[0] * 5] * B, [None] * B, 4, [1, 2])
    assert list(m._rowbatch) == keys and [len(idxs) for _, idxs in d.groups] == [k[0] for k in keys]
    assert sorted(d.at) == list(range(B))
    # the per-call override
    m2 = _fake_model(4)
    d2 = modeling._RowDriver(m2, B, 2.0, 1, 2, width=width)
    d2.begin([[0] * 5] * B, [None] * B, 4, [1, 2])
    assert list(m2._rowbatch) == keys


@pytest.mark.parametrize("width, slots, keys", [(4, 8, [(4, 0, "session", "side"), (4, 4, "session", "side")]), (8, 8, [(8, 0, "session", "side")]),
                                                (8, 16, [(8, 0, "session", "side"), (8, 8, "session", "side")]), (8, 3, [(3, 0, "session")])])
def test_width_reaches_the_session_driver(monkeypatch, width, slots, keys):
    from vibevoice_rocm_amd import rowbatch
    monkeypatch.setattr(rowbatch, "RowBatch", _FakeBatch)
    m = _fake_model(width)
    d = modeling._SessionDriver(m, slots, 1, 2, True)
    d.open(256, [1, 2])
    assert list(m._rowbatch) == keys and [len(idxs) for _, idxs in d.groups] == [k[0] for k in keys]
