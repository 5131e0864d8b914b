"""vv_linear's dispatch, decision by decision, against tests/golden/linear_route_sweep.json: what vv_linear_route answered for every case of
tools/route_sweep.py's grid BEFORE the weight-only formats' conditions moved into one refusal per kernel unit and one table (recorded at
that commit's parent; the half with the process-wide rows scratch on was recorded on the MI355X, the scratch being device memory).  Every
case must give the recorded rc and the recorded route name, and every refusal must leave a message.  Host decisions only: the arguments
are stand-in addresses, vv_linear is never called, nothing is launched."""
import collections
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import route_sweep  # noqa: E402

from conftest import GOLDEN  # noqa: E402

RECORD = route_sweep.load(os.path.join(GOLDEN, "linear_route_sweep.json"))
FORMATS = {2: "fp8", 3: "NF4", 4: "MXFP4", 5: "VV_MXFP4_FRAG", 6: "MXFP6"}      # vv_hip.h's wdt values of the weight-only formats


def _stage_counts(half):
    """refused cases per (weight-only wdt, stage of the record)"""
    rec = RECORD[half]
    n = collections.Counter()
    for case, r, stage in zip(route_sweep.cases(rec["min_rows"]), rec["results"], rec["stages"]):
        if r < 0 and case[0] in FORMATS:
            n[case[0], stage] += 1
            if case[0] == 2 and case[4] == 8:
                n["fp8 VV_LIN_W_FRAG", stage] += 1
    return n


def test_the_record_is_whole():
    """a trimmed record cannot pass empty: every axis value occurs, and every format has refused cases from each of the three stages that used to
    refuse them - shape / flags / scales ("a"), alignment ("l") and no kernel at that K ("k"); the fragment-major fp8 form meets the last two
    only with the scratch on"""
    off, on = RECORD["scratch_off"], RECORD["scratch_on"]
    assert len(off["results"]) == len(off["stages"]) == sum(1 for _ in route_sweep.cases()) > 50000
    assert len(on["results"]) == len(on["stages"]) == sum(1 for _ in route_sweep.cases(3)) > 30000
    seen = [set() for _ in range(5)]
    variants = set()
    for case in route_sweep.cases():
        for s, v in zip(seen, case[:5]):
            s.add(v)
        variants.add(route_sweep.VARIANTS.index(case[5]))
    assert [len(s) for s in seen] == [8, 7, 7, 2, 5] and len(variants) == len(route_sweep.VARIANTS) == 20
    n_off, n_on = _stage_counts("scratch_off"), _stage_counts("scratch_on")
    for wdt, name in FORMATS.items():
        for stage in "alk":
            assert n_off[wdt, stage] > 0, f"no {name} case refused at stage {stage!r} in the record"
    for stage in "alk":
        assert n_on["fp8 VV_LIN_W_FRAG", stage] > 0 and n_on[5, stage] > 0, stage
    assert any(r >= 0 for r in on["results"]) and any(r >= 0 for r in off["results"])


def test_every_decision_is_the_recorded_one():
    L, lib = route_sweep._lib(False)
    diffs = route_sweep.compare(RECORD["scratch_off"], route_sweep.sweep(L, lib, classify=False))
    assert not diffs, "\n".join(diffs)


@pytest.mark.gpu
def test_every_decision_with_the_rows_scratch_is_the_recorded_one():
    """the same with vv_tune("gemv_rows_scratch", 1), which allocates device memory (3 rows and more: fewer never look at it); run() switches
    it off again in a finally"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    diffs = route_sweep.compare(RECORD["scratch_on"], route_sweep.run(True, classify=False))
    assert not diffs, "\n".join(diffs)
