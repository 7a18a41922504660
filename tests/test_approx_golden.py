"""The Python restatement of ANUS::Qapprox (tests/approx_ref.py, on the oracle's scalar primitives) against what the
reference itself computed (tests/golden/ref_approx_0.jsonl.gz, written by tests/golden_src/ref_cases_approx.cpp), and the
conditions on the fixture that keep a green run from meaning "only the constant segment ran"."""
import math

import numpy as np
import pytest

import approx_ref as R

CASES = R.cases()


@pytest.mark.parametrize("j", CASES, ids=lambda j: j["name"])
def test_restatement_equals_reference(j):
    fx, segs = R.case_table(j)
    got = R.approx(j["X"], fx, segs)
    assert np.array_equal(got, np.asarray(j["Y"], dtype=np.int64)), j["name"]


@pytest.mark.parametrize("j", CASES, ids=lambda j: j["name"])
def test_every_segment_is_selected(j):
    fx, segs = R.case_table(j)
    hit = {R.select(int(x), fx, segs) for x in j["X"]}
    assert hit == set(range(len(segs))), (j["name"], sorted(hit))
    assert fx.raw_min in j["X"] and fx.raw_max in j["X"]
    for bp, _ in segs:          # each threshold inside the range: T - 1, T, T + 1
        T = R.threshold(bp, fx.fracBits)
        if T is not None and fx.raw_min < T < fx.raw_max:
            assert {T - 1, T, T + 1} <= set(j["X"]), (j["name"], bp)


def test_fixture_saturates_wraps_and_rounds_ties():
    seen = {}
    for j in CASES:
        fx, segs = R.case_table(j)
        ev = set()
        for x in j["X"]:
            R.approx_one(int(x), fx, segs, ev)
        seen[j["name"]] = ev
    assert all(any(k in ev for ev in seen.values()) for k in ("sat", "wrap", "tie")), seen


def test_fixture_holds_what_the_issue_lists():
    by = {j["name"]: R.case_table(j) for j in CASES}
    shape = lambda segs: [len(c) for _, c in segs]
    assert shape(by["probe_four_segments_mixed_modes"][1]) == [1, 3, 4, 1] and by["probe_four_segments_mixed_modes"][1][3][0] == math.inf
    bps = [bp for bp, _ in by["probe_unsorted_breakpoints"][1]]
    assert bps != sorted(bps)
    assert not by["probe_unsigned_x_rnd_inf_sat_zero"][0].isSigned
    fx, segs = by["uniform_sigmoid_8x_degree3"]
    assert shape(segs) == [4] * 8 and all([f for _, f in c] == [f for _, f in segs[0][1]] for _, c in segs)
    assert 8 in shape(by["degree7_segment"][1])
    assert shape(by["one_segment_degree2"][1]) == [3]
    assert by["negative_fracbits_x"][0].fracBits < 0
    assert by["x_of_40_value_bits"][0].W == 40
    # breakpoints that are no multiples of 2^-F (the ceil acts), and breakpoints outside x's range on both sides
    assert any((bp * 2.0 ** fx.fracBits) % 1 for fx, segs in by.values() for bp, _ in segs if not math.isinf(bp))
    assert by["breakpoint_above_range"][1][-1][0] * 16 > by["breakpoint_above_range"][0].raw_max
    assert by["breakpoint_below_range"][1][-1][0] * 16 < by["breakpoint_below_range"][0].raw_min
    assert sum(len(j["X"]) for j in CASES) > 1500
