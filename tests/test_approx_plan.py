"""CPU checks of the APPROX stage's planning (include/qgemul.h: qgemul_classify_epx): decisions and bits32 as far as the
C-ABI shows them, every refusal with its status, the old entry points' answer to op 5, and the ctypes mirrors of the ABI
structs against the C compiler's sizes (qgemul_sizeof)."""
import ctypes as C
import math

import pytest

import approx_ref as R
from qublas_amd import capi
from qublas_amd.desc import (EW_APPROX, Approx, Ew, Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, lower, lower_epilogue, lower_epilogue_cplx,
                             lower_epilogue_x)

ONE = Qu(1, 0, False)
X = Qu(7, 8)
FA = Qu(4, 10, True, RND.CONV, SAT.TCPL)
FB = Qu(3, 9, True, TRN.TCPL, SAT.ZERO)
TABLE = [(-2.0, [(-1234, FA)]), (0.3, [(700, FB), (-300, FA), (515, FA)]), (math.inf, [(-2047, FB)])]


def ident(c: Qu, n=64):
    return lower(c, ONE, c, n, 1, 1, mul_args=c)


def classify(c, stages, d, flags=0):
    ep, tabs = lower_epilogue_x(c, stages, d)
    return capi.classify_epx(ident(c), ep, tabs, flags)


def test_every_golden_table_is_supported_and_sizes_are_d():
    for j in R.cases():
        fx, segs = R.case_table(j)
        st, info = classify(fx, [Approx(segs)], fx)
        assert st == capi.QG_OK and info.supported == 1, (j["name"], info.reason)
        assert info.host_elem_bytes[2] == fx.host_bytes
        # the widest intermediate: at least a full product x * v of the longest segment, never beyond 62 bits
        assert fx.storage_bits <= info.max_bits <= 62, (j["name"], info.max_bits)


def test_max_bits_follows_the_horner_products():
    # x is 16 bits, the top coefficient 15 bits: the unrounded product needs up to 31 bits; a wider coefficient format widens it
    st, a = classify(X, [Approx([(0.0, [(1, FA), (1, FA)])])], X)
    st2, b = classify(X, [Approx([(0.0, [(1, FA), (1 << 29, Qu(20, 10))])])], X)
    assert st == st2 == capi.QG_OK
    assert a.max_bits <= 32 < b.max_bits


def test_chain_with_plain_stages_around_the_table():
    st, info = classify(Qu(15, 8), [Ew("mul", Qu(3, 4), Tags(24, 8), scalar=True, into=X), Approx(TABLE), Ew("mul", Qu(3, 4))], Qu(9, 3))
    assert st == capi.QG_OK, info.reason
    st, info = classify(X, [Approx(TABLE, into=Qu(4, 4)), Approx([(0.0, [(3, Qu(4, 4))])])], Qu(4, 4))   # two tables
    assert st == capi.QG_OK, info.reason


def refused(stages, d=X, c=X, mutate=None, tabs_mutate=None):
    ep, tabs = lower_epilogue_x(c, stages, d)
    if mutate:
        mutate(ep, tabs)
    st, info = capi.classify_epx(ident(c), ep, tabs)
    assert info.supported == 0 and info.reason, (st, info.reason)
    return st, info.reason.decode()


def test_refusals_invalid():
    E = capi.QG_EINVAL

    def n_seg(v):
        return lambda ep, tabs: setattr(tabs[0], "n_seg", v)
    assert refused([Approx(TABLE)], mutate=n_seg(0))[0] == E
    assert refused([Approx(TABLE)], mutate=n_seg(17))[0] == E

    def n_coef(v):
        return lambda ep, tabs: setattr(tabs[0].seg[1], "n_coef", v)
    assert refused([Approx(TABLE)], mutate=n_coef(0))[0] == E
    assert refused([Approx(TABLE)], mutate=n_coef(9))[0] == E
    st, why = refused([Approx([(math.nan, [(1, FA)])])])
    assert st == E and "NaN" in why
    st, why = refused([Approx([(0.0, [(1 << 14, FA)])])])          # FA holds [-2^14, 2^14 - 1]
    assert st == E and "coefficient" in why
    assert refused([Approx([(0.0, [(-(1 << 14) - 1, FA)])])])[0] == E
    assert refused([Approx([(0.0, [(-1, Qu(4, 4, False))])])])[0] == E   # unsigned format, negative raw value

    def wrong_r(ep, tabs):
        ep.stage[0].r = Qu(7, 8, True, TRN.TCPL, SAT.ZERO).c()       # differs in the OfMode only
    st, why = refused([Approx(TABLE)], mutate=wrong_r)
    assert st == E and "format" in why

    def drop_table(ep, tabs):
        tabs[0] = None
    assert refused([Approx(TABLE)], mutate=drop_table)[0] == E

    def surplus_table(ep, tabs):
        tabs[1] = tabs[0]
    assert refused([Approx(TABLE), Ew("add", FA)], mutate=surplus_table)[0] == E
    assert refused([Approx(TABLE)], mutate=surplus_table)[0] == E     # beyond the last stage

    def nonzero_e(ep, tabs):
        ep.stage[0].x_first = 1
    assert refused([Approx(TABLE)], mutate=nonzero_e)[0] == E


def test_refusals_unsupported():
    U = capi.QG_EUNSUPPORTED
    x54 = Qu(30, 24)
    st, why = refused([Approx([(0.0, [(1, Qu(4, 4))])])], d=x54, c=x54)
    assert st == U and "53" in why
    st, why = refused([Approx([(0.0, [(1, Qu(40, 23))])])])           # a Horner format of 63 value bits
    assert st == U and "62" in why
    st, why = refused([Approx([(0.0, [(1, Qu(30, 20)), (1 << 49, Qu(30, 20))])])], d=Qu(20, 20), c=Qu(20, 20))   # a 41-bit x times a 51-bit coefficient
    assert st == U and "62" in why
    # what the chain planner refuses anywhere: WRP::TCPL_SAT that can act inside the chain, RND over a 32-bit shift
    st, why = refused([Approx([(0.0, [(1, Qu(2, 2, True, TRN.TCPL, WRP.TCPL_SAT)), (16383, FA)])])])
    assert st == U and "TCPL_SAT" in why
    st, why = refused([Approx([(0.0, [(1, Qu(4, 0, True, RND.CONV, SAT.TCPL)), (3, Qu(4, 12))])])], d=Qu(10, 20), c=Qu(10, 20))
    assert st == U and "32" in why


def test_old_entry_points_still_reject_op_5():
    ep, tabs = lower_epilogue_x(X, [Approx(TABLE)], X)
    assert ep.stage[0].op == EW_APPROX == 5
    st, info = capi.classify_ep_status(ident(X), ep)
    assert st == capi.QG_EINVAL and info.reason == b"unknown element-wise op"
    cx = Qcomplex(X, X)
    epc = lower_epilogue_cplx(cx, [], cx)
    for p in range(2):
        epc.part[p].n_stages = 1
        epc.part[p].stage[0] = ep.stage[0]
    st, info = capi.classify_ep_status(lower(cx, cx, cx, 8, 8, 4), epc)
    assert st == capi.QG_EINVAL and info.reason == b"unknown element-wise op"
    # and a chain without APPROX stages is the same plan through either entry point
    e2, t2 = lower_epilogue_x(X, [Ew("add", FA)], X)
    assert bytes(e2) == bytes(lower_epilogue(X, [Ew("add", FA)], X)) and t2 == [None] * 4
    a, b = capi.classify_epx(ident(X), e2, t2), capi.classify_ep_status(ident(X), e2)
    assert a[0] == b[0] == capi.QG_OK and bytes(a[1]) == bytes(b[1])


def test_struct_sizes_match_the_c_side():
    for which, mirror in capi.SIZEOF_MIRRORS.items():
        assert capi.sizeof(which) == C.sizeof(mirror), (which, mirror.__name__)
    assert capi.sizeof(99) == 0
    assert C.sizeof(capi.qgemul_approx) == 8 + 16 * (16 + 8 * 8 + 8 * 8)


def test_one_shot_entry_accepts_a_null_operand_for_the_stage():
    """the stage reads no operand: the one-shot entry accepts a null E[k] for it (argument validation happens before any device work,
    so without a GPU the call gets as far as QG_ENOGPU, with one as far as running)"""
    import numpy as np
    ep, tabs = lower_epilogue_x(X, [Approx(TABLE)], X)
    d = ident(X, 4)
    xs = np.array([-600, -1, 77, 30000], dtype=np.int32)          # one input per segment, the middle one twice
    out = np.full(4, 12345, dtype=np.int32)
    try:
        capi.run_epx(d, ep, tabs, out, xs, np.ones(1, dtype=np.int32), [None])
    except capi.QgemulError as e:
        assert e.status == capi.QG_ENOGPU and (out == 12345).all()
    else:
        assert np.array_equal(out.astype(np.int64), R.approx(xs, X, TABLE))


def form(c, stages, d):
    ep, tabs = lower_epilogue_x(c, stages, d)
    return capi.approx_plan_form(ident(c), ep, tabs)


def test_bits32_uniform_and_thresholds():
    by = {j["name"]: R.case_table(j) for j in R.cases()}
    fx, segs = by["uniform_sigmoid_8x_degree3"]
    f = form(fx, [Approx(segs)], fx)
    assert f.bits32 == 1 and list(f.uniform) == [1, -1, -1, -1] and f.max_bits <= 32
    assert list(f.threshold[0])[:7] == [int(bp * 4096) for bp, _ in segs[:7]] and f.threshold[0][7] == fx.raw_max + 1
    # one level's QuMode changed in one segment: the general form, same arithmetic width
    odd = [(bp, list(c)) for bp, c in segs]
    a, q = odd[3][1][1]
    odd[3][1][1] = (a, Qu(q.intBits, q.fracBits, q.isSigned, RND.ZERO, q.OfMode))
    g = form(fx, [Approx(odd)], fx)
    assert g.bits32 == 1 and g.uniform[0] == 0
    # segments of different lengths: general
    assert form(X, [Approx(TABLE)], X).uniform[0] == 0
    # 40 value bits: 64-bit arithmetic; a 32-bit-storage x as well (the clamped threshold 2^31 is no int32)
    fx40, s40 = by["x_of_40_value_bits"]
    assert form(fx40, [Approx(s40)], fx40).bits32 == 0
    assert form(Qu(15, 16), [Approx([(0.0, [(1, Qu(15, 16))])])], Qu(15, 16)).bits32 == 0
    assert form(Qu(14, 16), [Approx([(0.0, [(1, Qu(14, 16))])])], Qu(14, 16)).bits32 == 1
    # the ceil, and the clamps of breakpoints outside the range, +-inf included
    for j in R.cases():
        fx, segs = R.case_table(j)
        thr = list(form(fx, [Approx(segs)], fx).threshold[0])
        for s, (bp, _) in enumerate(segs[:-1]):
            T = R.threshold(bp, fx.fracBits)
            want = fx.raw_max + 1 if T is None else min(max(T, fx.raw_min), fx.raw_max + 1)
            assert thr[s] == want, (j["name"], s)
        assert all(t == fx.raw_max + 1 for t in thr[len(segs) - 1:])
    thr = list(form(X, [Approx([(-math.inf, [(1, FA)]), (0.3, [(2, FA)]), (5e-324, [(3, FA)]), (-5e-324, [(4, FA)]), (0.0, [(5, FA)])])], X).threshold[0])
    assert thr[:4] == [X.raw_min, 77, 1, 0]


# ---- the Python lowering and both C++ headers produce the same bytes for the same chains (tests/binding/*approx_probe.cpp) ----
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REF_INC = os.environ.get("REF_INC", "/root/reference/include")


def python_chains():
    FC = Qu(2, 8, True, RND.ZERO, WRP.TCPL)
    ct, s34, q44 = Qu(15, 8), Qu(3, 4), Qu(4, 4)
    seg0 = (-2.0, [(-1234, FA)])
    seg1 = (0.3, [(700, FB), (-300, FC), (515, FA)])
    seg2 = (1e30, [(-2047, FB), (9000, FA)])
    out = {}
    for name, c, stages, d in (
            ("scale_approx_mul", ct, [Ew("mul", s34, Tags(24, 8), scalar=True, into=X), Approx([seg0, seg1, seg2], into=q44), Ew("mul", s34)],
             Qu(9, 3, True, RND.NEG_INF, SAT.SMGN)),
            ("approx_alone", X, [Approx([seg1])], X)):
        ep, tabs = lower_epilogue_x(c, stages, d)
        out[name] = {"ep": bytes(ep).hex(), "ax": [None if t is None else bytes(t).hex() for t in tabs]}
    return out


def _probe(tmp_path, src, extra=()):
    exe = tmp_path / os.path.splitext(src)[0]
    subprocess.check_call([CLANG, "-std=c++23", "-O0", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "binding"), *extra,
                           os.path.join(ROOT, "tests", "binding", src), "-o", str(exe)])
    lines = [json.loads(l) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines()]
    return {l["name"]: {"ep": l["ep"], "ax": l["ax"]} for l in lines}


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_lowers_to_the_same_bytes(tmp_path):
    assert _probe(tmp_path, "amd_header_approx_probe.cpp") == python_chains()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_reference_binding_lowers_to_the_same_bytes(tmp_path):
    if not os.path.exists(os.path.join(REF_INC, "QuBLAS.h")):
        pytest.skip("the reference header is not on this machine")
    assert _probe(tmp_path, "ref_binding_approx_probe.cpp", ["-I" + REF_INC]) == python_chains()
