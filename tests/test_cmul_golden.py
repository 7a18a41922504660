"""The Python restatement of the reference's complex x complex Qmul (tests/cmul_ref.py, on the oracle's scalar primitives) against
what the reference itself computed (tests/golden/ref_cplx_cmul_0.jsonl.gz, written by tests/golden_src/ref_cases_cplx_cmul.cpp); the
Python lowering (desc.lower_epilogue_cplx_x) against the formats the reference's own types report in the same records; and the
conditions on the fixture that keep a green run from meaning "everything saturated"."""
import numpy as np
import pytest

import cmul_ref as R
from qublas_amd.desc import (CMUL_BASIC, CMUL_TF, EW_CMUL, RND, SAT, TRN, WRP, BasicComplexMul, EwC, Qcomplex, Qu, Tags, TFComplexMul,
                             lower_epilogue_cplx_x)

CASES = R.cases()
BY = {j["name"]: j for j in CASES}

# the generator's types and tags, restated (tests/golden_src/ref_cases_cplx_cmul.cpp)
X64, E35 = Qu(6, 4), Qu(3, 5)
R63, R6N3 = Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL)
R54, R32, S22, U44 = Qu(5, 4), Qu(3, 2), Qu(2, 2), Qu(4, 4, False)
R104, R82Z = Qu(10, 4, True, RND.CONV, SAT.SMGN), Qu(8, 2, True, TRN.TCPL, SAT.ZERO)
R73W, R91S = Qu(7, 3, True, RND.ZERO, WRP.TCPL), Qu(9, 1, True, TRN.SMGN, SAT.SMGN)
CX, CE, C5, CB, CU = Qcomplex(X64, X64), Qcomplex(E35, E35), Qcomplex(R63, R6N3), Qcomplex(R54, R32), Qcomplex(U44, R54)
CD, CQ, CW = Qcomplex(R104, R82Z), Qcomplex(R73W, R91S), Qcomplex(Qu(20, 6), Qu(20, 6))
CWX, CWE, CWD = Qcomplex(Qu(24, 12), Qu(24, 12)), Qcomplex(Qu(10, 12), Qu(10, 12)), Qcomplex(Qu(40, 18), Qu(40, 18))
T_AC = Tags(intBits=8, fracBits=3, QuMode=RND.POS_INF)
T_BD = Tags(fracBits=2, QuMode=RND.NEG_INF, OfMode=SAT.ZERO)
T_AD = Tags(fracBits=1, QuMode=RND.ZERO, OfMode=WRP.TCPL)
T_BC = Tags(fracBits=2, QuMode=RND.INF, OfMode=SAT.SMGN)
T_ACBD = Tags(intBits=5, fracBits=2, QuMode=RND.CONV)
T_ADBC = Tags(intBits=5, fracBits=1, QuMode=TRN.SMGN, OfMode=WRP.TCPL)
T_AB = Tags(intBits=6, fracBits=3, QuMode=RND.INF)
T_CD = Tags(intBits=3, fracBits=4, QuMode=RND.ZERO, OfMode=WRP.TCPL)
T_BA = Tags(intBits=2, fracBits=0, OfMode=SAT.ZERO)
T_ABC = Tags(intBits=8, fracBits=3, QuMode=RND.CONV)
T_CDB = Tags(intBits=7, fracBits=2, QuMode=RND.NEG_INF, OfMode=SAT.SMGN)
T_BAD = Tags(intBits=6, fracBits=4, QuMode=RND.POS_INF, OfMode=SAT.ZERO)
T_ABT = Tags(intBits=7, fracBits=2, QuMode=TRN.SMGN)
T_BCT = Tags(intBits=6, fracBits=3, OfMode=WRP.TCPL)
TF8 = TFComplexMul(abT=T_AB, cdT=T_CD, baT=T_BA, abcT=T_ABC, cdbT=T_CDB, badT=T_BAD, ABT=T_ABT, BCT=T_BCT)
FP = Tags(FullPrec=True)


def one(c, e, d, tags=None, x_first=True, scalar=False):
    return c, [EwC("mul", e, tags=tags, x_first=x_first, scalar=scalar)], d


LOWERINGS = {
    "basic_no_tags": one(CX, CE, CD),
    "basic_no_tags_efirst": one(CX, CE, CD, x_first=False),
    "basic_acT": one(CX, CE, CD, BasicComplexMul(acT=T_AC)),
    "basic_bdT": one(CX, CE, CD, BasicComplexMul(bdT=T_BD)),
    "basic_adT": one(CX, CE, CD, BasicComplexMul(adT=T_AD)),
    "basic_bcT": one(CX, CE, CD, BasicComplexMul(bcT=T_BC)),
    "basic_acbdT": one(CX, CE, CQ, BasicComplexMul(acbdT=T_ACBD)),
    "basic_adbcT": one(CX, CE, CQ, BasicComplexMul(adbcT=T_ADBC)),
    "basic_all_six_efirst": one(CX, CE, CQ, BasicComplexMul(T_AC, T_BD, T_AD, T_BC, T_ACBD, T_ADBC), x_first=False),
    "basic_loose_tags": one(CX, CE, CD, BasicComplexMul(loose=Tags(intBits=7, fracBits=3, QuMode=RND.CONV))),
    "tf_no_tags": one(CX, CE, CD, TFComplexMul()),
    "tf_baT_only": one(CX, CE, CD, TFComplexMul(baT=T_BA)),
    "tf_no_tags_efirst": one(CX, CE, CD, TFComplexMul(), x_first=False),
    "tf_all_eight": one(CX, CE, CQ, TF8),
    "tf_all_eight_efirst": one(CX, CE, CQ, TF8, x_first=False),
    "tf_loose_tags": one(CX, CE, CD, TFComplexMul(loose=Tags(intBits=8, fracBits=2, QuMode=RND.NEG_INF, OfMode=SAT.SMGN))),
    "basic_scalar": one(CX, CE, CD, BasicComplexMul(acT=T_AC, acbdT=T_ACBD), scalar=True),
    "tf_scalar_efirst": one(CX, CB, CQ, TFComplexMul(abcT=T_ABC, BCT=T_BCT), x_first=False, scalar=True),
    "mixed_parts_basic": one(C5, CB, CD),
    "mixed_parts_tf_unsigned_efirst": one(C5, CU, CQ, TFComplexMul(), x_first=False),
    "cmul_into_then_real_scale": (CX, [EwC("mul", CE, tags=BasicComplexMul(acT=T_AC), into=CQ), EwC("mul", S22, scalar=True)], CD),
    "add_cmul_mul_by_real": (CX, [EwC("add", CB, into=CW), EwC("mul", CE, tags=TFComplexMul(abcT=T_ABC), into=C5),
                                  EwC("mul", R32, imag_tags=R91S, x_first=False)], CQ),
    "cmul_then_cmul": (CX, [EwC("mul", CE, into=CX), EwC("mul", CB, tags=TFComplexMul(), x_first=False, scalar=True)], CD),
    "wide_basic_fullprec": one(CWX, CWE, CWD, BasicComplexMul(FP, FP, FP, FP, FP, FP)),
    "wide_tf_fullprec_efirst": one(CWX, CWE, CWD, TFComplexMul(abcT=FP, cdbT=FP, badT=FP), x_first=False),
}


def run(j, ev=None):
    epc, cx, c, _ = R.case_chain(j)
    Ere, Eim = R.case_operands(j)
    return R.chain(epc, cx, c, j["Xre"], j["Xim"], Ere, Eim, ev)


@pytest.mark.parametrize("j", CASES, ids=lambda j: j["name"])
def test_restatement_equals_reference(j):
    re, im = run(j)
    assert np.array_equal(re, np.asarray(j["Dre"], dtype=np.int64)), j["name"]
    assert np.array_equal(im, np.asarray(j["Dim"], dtype=np.int64)), j["name"]


def test_every_record_has_its_lowering():
    assert sorted(LOWERINGS) == sorted(BY)


@pytest.mark.parametrize("name", sorted(LOWERINGS))
def test_python_lowering_equals_the_references_types(name):
    """byte for byte: the stage records, the destination, e_complex, and every slot of every qgemul_cmul"""
    c, stages, d = LOWERINGS[name]
    epc, cx = lower_epilogue_cplx_x(c, stages, d)
    ref_epc, ref_cx, ref_c, ref_d = R.case_chain(BY[name])
    assert (c, d) == (ref_c, ref_d)
    assert bytes(epc) == bytes(ref_epc), name
    for k in range(len(cx)):
        assert (cx[k] is None) == (ref_cx[k] is None), (name, k)
        if cx[k] is not None:
            assert bytes(cx[k]) == bytes(ref_cx[k]), (name, k)


def test_baT_is_never_honoured_and_badT_cdbT_are_crossed():
    a, b = BY["tf_no_tags"], BY["tf_baT_only"]
    assert a["stages"][0]["mul"] == b["stages"][0]["mul"] and a["Dre"] == b["Dre"] and a["Dim"] == b["Dim"]
    m = BY["tf_all_eight"]["stages"][0]["mul"]
    assert m[R.T_BA] == [6, 4, 1, TRN.TCPL, SAT.TCPL]                  # (b - a): the default merge, not baT's Qu<2, 0, SAT::ZERO>
    assert m[R.T_B] == [6, 4, 1, RND.POS_INF, SAT.ZERO]                # B = (c + d) b carries badT
    assert m[R.T_C] == [7, 2, 1, RND.NEG_INF, SAT.SMGN]                # C = (b - a) d carries cdbT


def test_the_order_matters():
    """TF treats its arguments differently; Basic without tags on parts of one format is symmetric, so its pair agrees"""
    x, e = BY["tf_no_tags"], BY["tf_no_tags_efirst"]
    assert x["Xre"] == e["Xre"] and x["stages"][0]["Ere"] == e["stages"][0]["Ere"]
    assert x["Dre"] != e["Dre"] or x["Dim"] != e["Dim"]
    x, e = BY["basic_no_tags"], BY["basic_no_tags_efirst"]
    assert x["Dre"] == e["Dre"] and x["Dim"] == e["Dim"]


def test_fixture_ties_saturates_and_wraps_and_is_not_hidden_by_it():
    seen = {}
    for j in CASES:
        ev = set()
        run(j, ev)
        seen[j["name"]] = ev
        assert len(set(j["Dre"])) > 8 and len(set(j["Dim"])) > 8, j["name"]
    assert all(any(k in ev for ev in seen.values()) for k in ("sat", "wrap", "tie")), seen
    # the sub-operations between them carry all seven QuModes and the four OfModes
    modes = [f for j in CASES for s in j["stages"] if s["op"] == EW_CMUL for f in s["mul"][:8 if s["cmul"] == CMUL_TF else 6]]
    assert {f[3] for f in modes} == set(range(7)) and {f[4] for f in modes} == set(range(4))


def test_fixture_holds_what_the_issue_lists():
    kinds = {(s["cmul"], s["x_first"], s["scalar"]) for j in CASES for s in j["stages"] if s["op"] == EW_CMUL}
    assert {(CMUL_BASIC, 1, 0), (CMUL_BASIC, 0, 0), (CMUL_TF, 1, 0), (CMUL_TF, 0, 0), (CMUL_BASIC, 1, 1), (CMUL_TF, 0, 1)} <= kinds
    assert BY["mixed_parts_basic"]["c"][0] != BY["mixed_parts_basic"]["c"][1] and BY["mixed_parts_basic"]["c"][1][1] < 0
    s = BY["cmul_into_then_real_scale"]["stages"][0]
    assert s["t"] != s["r"]                                            # an `into` conversion
    assert [s["op"] for s in BY["add_cmul_mul_by_real"]["stages"]] == [1, EW_CMUL, 3]
    assert [s["op"] for s in BY["cmul_then_cmul"]["stages"]] == [EW_CMUL, EW_CMUL]
    for name in ("wide_basic_fullprec", "wide_tf_fullprec_efirst"):    # 8-byte parts, sub-operations of 59 .. 61 storage bits
        j = BY[name]
        assert 1 + sum(j["c"][0][:2]) > 32 and max(1 + f[0] + f[1] for f in j["stages"][0]["mul"]) >= 59
    assert 20 <= len(CASES) <= 30 and all(64 <= j["n"] <= 256 for j in CASES)
