"""CPU checks of the CMUL stage's planning (include/qgemul.h: qgemul_classify_epcx, qgemul_cmul_plan_form): the golden chains are
accepted, every refusal comes with its status, the older entry points keep refusing op 6, the pass's arithmetic width is 32 bits
exactly where every part of the chain allows it, and the ctypes mirrors of the ABI structs have the C compiler's sizes."""
import copy
import ctypes as C

import pytest

import cmul_ref as R
from qublas_amd import capi
from qublas_amd.desc import (CMUL_TF, EW_ADD, EW_CMUL, EW_MUL, QG_MAX_EW, BasicComplexMul, Ew, EwC, Qcomplex, Qu, RND, SAT, WRP, Tags, TFComplexMul,
                             host_layout, lower, lower_epilogue, lower_epilogue_cplx_x, qgemul_cmul, qgemul_epilogue_cplx)

ONE = Qu(1, 0, False)
CONE = Qcomplex(ONE, ONE)
X = Qcomplex(Qu(6, 4), Qu(6, 4))
E = Qcomplex(Qu(3, 5), Qu(3, 5))
D = Qcomplex(Qu(8, 4), Qu(8, 4))


def ident(c: Qcomplex, n=64):
    return lower(c, CONE, c, n, 1, 1, mul_args=BasicComplexMul(acT=c.real, bdT=c.imag, adT=c.real, bcT=c.imag, acbdT=c.real, adbcT=c.imag))


def classify(c, stages, d, mutate=None):
    epc, cx = lower_epilogue_cplx_x(c, stages, d)
    if mutate:
        mutate(epc, cx)
    st, info = capi.classify_epcx(ident(c), epc, cx)
    st2, form = capi.cmul_plan_form(ident(c), epc, cx)
    assert st2 == st, (st, st2, info.reason)
    return st, info, form


@pytest.mark.parametrize("j", R.cases(), ids=lambda j: j["name"])
def test_every_golden_chain_is_supported_and_sizes_are_d(j):
    epc, cx, c, d = R.case_chain(j)
    st, info = capi.classify_epcx(ident(c, j["n"]), epc, cx)
    assert st == capi.QG_OK and info.supported == 1, (j["name"], info.reason)
    assert info.host_elem_bytes[2] == host_layout(d)[0]
    st, form = capi.cmul_plan_form(ident(c, j["n"]), epc, cx)
    assert st == capi.QG_OK and form.has_cmul == 1
    # the widest intermediate: at least a full product of two parts, never beyond 62 bits; 32-bit arithmetic exactly for the narrow ones
    assert c.real.storage_bits < form.max_bits <= 62 and form.max_bits == info.max_bits
    assert form.bits32 == (0 if j["name"].startswith("wide_") else 1), (j["name"], form.max_bits)


def test_bits32_goes_off_with_any_wide_piece():
    narrow = [EwC("mul", E)]
    assert classify(X, narrow, D)[2].bits32 == 1
    # a CMUL node beyond 32 bits (a full-precision product of 20-bit parts), the other chain's destination, a plain stage's operand,
    # an 8-byte operand container, C itself
    wide_node = [EwC("mul", Qcomplex(Qu(10, 9), Qu(3, 5)), tags=BasicComplexMul(acT=Tags(FullPrec=True)))]
    st, _, form = classify(Qcomplex(Qu(10, 9), Qu(6, 4)), wide_node, D)
    assert st == capi.QG_OK and form.bits32 == 0 and form.max_bits > 32
    assert classify(X, narrow, Qcomplex(Qu(8, 4), Qu(30, 4)))[2].bits32 == 0
    assert classify(X, narrow + [EwC("add", Qu(30, 4), scalar=True)], D)[2].bits32 == 0
    assert classify(X, [EwC("mul", Qcomplex(Qu(3, 5), Qu(20, 13)), tags=BasicComplexMul(loose=Qu(6, 5)))], D)[2].bits32 == 0
    assert classify(Qcomplex(Qu(6, 4), Qu(30, 4)), [EwC("mul", E, tags=BasicComplexMul(loose=Qu(6, 5)))], D)[2].bits32 == 0
    # a chain without a CMUL stage takes the two-launch pass: no CMUL form
    st, _, form = classify(X, [EwC("add", E)], D)
    assert st == capi.QG_OK and form.has_cmul == 0


def refused(stages, mutate, c=X, d=D):
    st, info, _ = classify(c, stages, d, mutate)
    assert info.supported == 0 and info.reason, (st, info.reason)
    return st, info.reason.decode()


def part(epc, p, k=0):
    return epc.part[p].stage[k]


def test_refusals_invalid():
    EI = capi.QG_EINVAL
    one = [EwC("mul", E, tags=TFComplexMul())]

    def set_(p, field, v):
        return lambda epc, cx: setattr(part(epc, p), field, v)
    # op 6 in one part only (either one)
    assert refused(one, set_(0, "op", EW_MUL))[0] == EI
    assert refused(one, set_(1, "op", EW_ADD))[0] == EI
    # x_first / e_scalar differ between the parts
    assert refused(one, set_(1, "x_first", 0))[0] == EI
    assert refused(one, set_(0, "e_scalar", 1))[0] == EI
    # the operand is declared real
    assert refused(one, lambda epc, cx: epc.e_complex.__setitem__(0, 0))[0] == EI
    # a missing record, a surplus one (on a plain stage, beyond the last stage, in a chain without any CMUL stage)
    assert refused(one, lambda epc, cx: cx.__setitem__(0, None))[0] == EI
    two = [EwC("add", E), EwC("mul", E)]
    assert refused(two, lambda epc, cx: cx.__setitem__(0, copy.copy(cx[1])))[0] == EI
    assert refused(one, lambda epc, cx: cx.__setitem__(QG_MAX_EW - 1, copy.copy(cx[0])))[0] == EI
    assert refused([EwC("add", E)], lambda epc, cx: cx.__setitem__(0, qgemul_cmul()))[0] == EI
    # cmul neither Basic nor TF
    for v in (0, 3, 255):
        assert refused(one, lambda epc, cx, v=v: setattr(cx[0], "cmul", v))[0] == EI
    # r unequal to the RE / IM slot, in each of the five fields, in either part
    for p in range(2):
        for field, v in (("I", 9), ("F", 1), ("S", 0), ("Q", RND.CONV), ("O", SAT.ZERO)):
            def bend(epc, cx, p=p, field=field, v=v):
                setattr(part(epc, p).r, field, v)
            st, why = refused(one, bend)
            assert st == EI and "RE / IM" in why, (p, field, why)
    # unknown op codes stay unknown
    assert refused(one, lambda epc, cx: (setattr(part(epc, 0), "op", 7), setattr(part(epc, 1), "op", 7)))[0] == EI
    assert refused(one, lambda epc, cx: (setattr(part(epc, 0), "op", 5), setattr(part(epc, 1), "op", 5)))[0] == EI


def test_refusals_unsupported():
    EU = capi.QG_EUNSUPPORTED
    # a sub-operation beyond 62 bits: the full product of two 37-bit parts; a slot format of 70 value bits
    W = Qcomplex(Qu(24, 12), Qu(24, 12))
    st, why = refused([EwC("mul", W, tags=BasicComplexMul(loose=Qu(30, 12)))], None, c=W, d=W)
    assert st == EU and "62" in why, why
    st, why = refused([EwC("mul", E, tags=BasicComplexMul(acT=Qu(40, 30)))], None)
    assert st == EU and "62" in why, why
    # what every chain refuses holds for each node: WRP::TCPL_SAT that can act, RND over a 32-bit shift, unsigned WRP::TCPL of 32 bits
    st, why = refused([EwC("mul", E, tags=BasicComplexMul(bdT=Qu(2, 2, True, RND.CONV, WRP.TCPL_SAT)))], None)
    assert st == EU and "TCPL_SAT" in why, why
    W2 = Qcomplex(Qu(4, 20), Qu(4, 20))
    st, why = refused([EwC("mul", W2, tags=TFComplexMul(abcT=Qu(8, 8, True, RND.POS_INF)))], None, c=W2, d=D)
    assert st == EU and "32/64-bit shift" in why, why
    st, why = refused([EwC("mul", E, tags=TFComplexMul(ABT=Qu(4, 28, False, RND.CONV, WRP.TCPL)))], None)
    assert st == EU and "unsigned WRP::TCPL" in why, why
    # ... and a TCPL_SAT that cannot act is a clamp that never fires
    st, info, _ = classify(X, [EwC("mul", E, tags=BasicComplexMul(acT=Qu(12, 9, True, RND.CONV, WRP.TCPL_SAT)))], D)
    assert st == capi.QG_OK, info.reason


def test_the_older_entry_points_refuse_op_6():
    epc, cx = lower_epilogue_cplx_x(X, [EwC("mul", E)], D)
    st, info = capi.classify_ep_status(ident(X), epc)                     # qgemul_classify_epc
    assert st == capi.QG_EINVAL and b"unknown element-wise op" in info.reason
    # a real GEMM: op 6 in a qgemul_epilogue (_ep and _epx), and a complex chain on it (_epcx)
    c = Qu(6, 4)
    dr = lower(c, ONE, c, 16, 1, 1, mul_args=c)
    ep = lower_epilogue(c, [Ew("mul", Qu(3, 5))], c)
    ep.stage[0].op = EW_CMUL
    assert capi.classify_ep_status(dr, ep)[0] == capi.QG_EINVAL
    assert capi.classify_epx(dr, ep, [None] * QG_MAX_EW)[0] == capi.QG_EINVAL
    assert capi.classify_epcx(dr, epc, cx)[0] == capi.QG_EINVAL
    # null arguments
    L = capi.lib()
    assert L.qgemul_classify_epcx(C.byref(ident(X)), C.byref(epc), None, 0, C.byref(capi.qgemul_info())) == capi.QG_EINVAL
    assert L.qgemul_cmul_plan_form(C.byref(ident(X)), None, capi._cmuls(cx), C.byref(capi.qgemul_cmul_form())) == capi.QG_EINVAL


def test_a_chain_without_cmul_plans_as_under_epc():
    """the _epcx entry with no CMUL stage and no record answers what _epc answers, field by field"""
    from qublas_amd.desc import lower_epilogue_cplx
    stages = [EwC("add", E), EwC("mul", Qu(2, 2), scalar=True)]
    epc = lower_epilogue_cplx(X, stages, D)
    epx, cx = lower_epilogue_cplx_x(X, stages, D)
    assert bytes(epc) == bytes(epx) and cx == [None] * QG_MAX_EW
    (s1, a), (s2, b) = capi.classify_ep_status(ident(X), epc), capi.classify_epcx(ident(X), epx, cx)
    assert s1 == s2 == capi.QG_OK and bytes(a) == bytes(b)


def test_abi_struct_sizes():
    assert capi.SIZEOF_MIRRORS[10] is qgemul_cmul
    for which, mirror in capi.SIZEOF_MIRRORS.items():
        assert capi.sizeof(which) == C.sizeof(mirror), (which, mirror.__name__)
    assert C.sizeof(qgemul_cmul) == 8 + 8 * 8 and capi.sizeof(11) == 0
    assert C.sizeof(qgemul_epilogue_cplx) == capi.sizeof(7)
    assert CMUL_TF == 2 and EW_CMUL == 6


def test_the_lock_step_planner_under_sanitizers(tmp_path):
    """qg_analyze_epcx under ASan + UBSan on 60 000 random chains, a third of them malformed on purpose (tests/san/cmul_plan_san_driver.cpp)"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cmul_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(root, "tests", "san", "cmul_plan_san_driver.cpp"), os.path.join(root, "qublas_amd", "csrc", "qg_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "ERROR" not in r.stderr, (r.stdout[-500:], r.stderr[-2000:])
    ok, inv, uns = (int(x) for x in r.stdout.split()[1::2])
    assert ok > 1000 and inv > 1000 and uns > 1000, r.stdout       # all three answers are exercised
