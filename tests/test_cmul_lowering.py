"""The three lowerings of a complex chain with a complex x complex multiplication — qublas_amd/desc.py, include/QuBLAS_amd.h and
include/qgemul_reference_binding.hpp on the reference's own header — produce byte-identical qgemul_epilogue_cplx + qgemul_cmul for
a Basic and a TF chain (tests/binding/*cmul_probe.cpp: the same chains, spelled once in cmul_probe_common.hpp); the planner accepts
them."""
import json
import os
import subprocess

import pytest

from qublas_amd import capi
from qublas_amd.desc import (BasicComplexMul, EwC, Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, lower, lower_epilogue_cplx_x)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REF_INC = os.environ.get("REF_INC", "/root/reference/include")

X64, E35 = Qu(6, 4), Qu(3, 5)
R63, R6N3 = Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL)
R54, R32, R206 = Qu(5, 4), Qu(3, 2), Qu(20, 6)
R73W, R91S = Qu(7, 3, True, RND.ZERO, WRP.TCPL), Qu(9, 1, True, TRN.SMGN, SAT.SMGN)
CX, CE, C5, CB, CW, CQ = Qcomplex(X64, X64), Qcomplex(E35, E35), Qcomplex(R63, R6N3), Qcomplex(R54, R32), Qcomplex(R206, R206), Qcomplex(R73W, R91S)
CHAINS = {
    "basic_chain": (CX, [EwC("add", CB, into=CW),
                         EwC("mul", CE, tags=BasicComplexMul(acT=Tags(8, 3, QuMode=RND.POS_INF), adbcT=Tags(5, 1, QuMode=TRN.SMGN, OfMode=WRP.TCPL),
                                                             loose=Tags(fracBits=2, QuMode=RND.CONV)), into=C5),
                         EwC("mul", R32, imag_tags=R91S, x_first=False, scalar=True)], CQ),
    "tf_rmul_scalar_then_plain": (C5, [EwC("mul", CB, tags=TFComplexMul(baT=Tags(2, 0, OfMode=SAT.ZERO), abcT=Tags(8, 3, QuMode=RND.CONV),
                                                                         cdbT=Tags(7, 2, QuMode=RND.NEG_INF, OfMode=SAT.SMGN),
                                                                         badT=Tags(6, 4, QuMode=RND.POS_INF, OfMode=SAT.ZERO), BCT=Tags(6, 3, OfMode=WRP.TCPL)),
                                           x_first=False, scalar=True),
                                       EwC("mul", CE)], CQ),
}


def python_chains():
    out = {}
    for name, (c, stages, d) in CHAINS.items():
        epc, cx = lower_epilogue_cplx_x(c, stages, d)
        out[name] = {"ep": bytes(epc).hex(), "cx": [None if t is None else bytes(t).hex() for t in cx]}
    return out


def _probe(tmp_path, src, extra=()):
    exe = tmp_path / os.path.splitext(src)[0]
    subprocess.check_call([CLANG, "-std=c++23", "-O0", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "binding"), *extra,
                           os.path.join(ROOT, "tests", "binding", src), "-o", str(exe)])
    lines = [json.loads(l) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines()]
    return {l["name"]: {"ep": l["ep"], "cx": l["cx"]} for l in lines}


def test_the_planner_accepts_both_chains_and_they_hold_what_they_should():
    for name, (c, stages, d) in CHAINS.items():
        epc, cx = lower_epilogue_cplx_x(c, stages, d)
        ident = lower(c, Qcomplex(Qu(1, 0, False), Qu(1, 0, False)), c, 8, 1, 1,
                      mul_args=BasicComplexMul(acT=c.real, bdT=c.imag, adT=c.real, bcT=c.imag, acbdT=c.real, adbcT=c.imag))
        st, info = capi.classify_epcx(ident, epc, cx)
        assert st == capi.QG_OK, (name, info.reason)
    _, cx = lower_epilogue_cplx_x(*CHAINS["basic_chain"][:2], CHAINS["basic_chain"][2])
    assert [t is not None for t in cx] == [False, True, False, False] and cx[1].cmul == 1
    _, cx = lower_epilogue_cplx_x(*CHAINS["tf_rmul_scalar_then_plain"][:2], CHAINS["tf_rmul_scalar_then_plain"][2])
    assert [t is not None for t in cx] == [True, True, False, False] and (cx[0].cmul, cx[1].cmul) == (2, 1)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_lowers_to_the_same_bytes(tmp_path):
    assert _probe(tmp_path, "amd_header_cmul_probe.cpp") == python_chains()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_reference_binding_lowers_to_the_same_bytes(tmp_path):
    if not os.path.exists(os.path.join(REF_INC, "QuBLAS.h")):
        pytest.skip("the reference header is not on this machine")
    assert _probe(tmp_path, "ref_binding_cmul_probe.cpp", ["-I" + REF_INC]) == python_chains()
