"""Qgemul with one real and one complex operand (QG_CMUL_REAL_A / QG_CMUL_REAL_B, include/qgemul.h) without a GPU:
  * the checker of tests/mixed_ref.py — part p of a mixed descriptor as a real Qgemul through the unchanged oracle — equals the reference
    itself on every golden record (tests/golden/ref_mixed_0, written by tests/golden_src/ref_cases_mixed.cpp from the reference's header);
  * the Python lowering and the standalone header (include/QuBLAS_amd.h, through tests/binding/amd_header_mixed_probe.cpp) reproduce
    the formats the reference's own types report in those records;
  * qgemul_classify answers a mixed descriptor: class, kernel, step form, ops and per-operand host layouts;
  * the new QG_EINVAL cases, and the clean refusals (QG_EUNSUPPORTED, "mixed real-complex") of chains, batched and grouped plans and
    the sharded run;
  * the planner under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program (tests/san/mixed_plan_san_driver.cpp)
    on every golden descriptor plus random and malformed mixed ones, verdicts equal to the product library's;
  * the compiler's resource report of the mixed tree kernel: no instantiation uses scratch."""
import ctypes as C
import os
import random
import re
import struct
import subprocess

import numpy as np
import pytest

import mixed_ref as R
from qublas_amd import capi
from qublas_amd.desc import (CLASS_LINEAR, CLASS_TREE, CMUL_REAL_A, CMUL_REAL_B, Qcomplex, Qu, RealComplexMul, RND, SAT, TRN, WRP, Tags, desc_to_dict, lower,
                             qgemul_epilogue, qgemul_epilogue_cplx)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
CASES = R.cases()

E43, E88 = Qu(4, 3), Qu(8, 8)
C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
C88 = Qcomplex(Qu(8, 8), Qu(7, 5))
CC = Qcomplex(Qu(14, 3), Qu(14, 3))
RI = RealComplexMul(realT=Qu(12, 6), imagT=Tags(10, 0))
CRI = Qcomplex(Qu(18, 6), Qu(16, 0))
QQ = (Qu(7, 5, True, RND.ZERO, SAT.SMGN), Qu(9, -1, True, TRN.SMGN, WRP.TCPL))
L12 = [Qcomplex(Qu(8, 4, True, RND.CONV, SAT.SMGN), Qu(9, 1, True, TRN.SMGN, SAT.ZERO)), Qcomplex(Qu(12, 2, True, RND.ZERO), Qu(12, 3, True, RND.INF, WRP.TCPL))]
CWD = Qcomplex(Qu(20, 4), Qu(20, 3))
# the tags of tests/golden_src/ref_cases_mixed.cpp, case by case: name prefix -> (real element, complex element, C, lowering keywords)
TAGS = {
    "default_narrowC": (E43, C5, C5, {}),
    "default": (E43, C5, CC, {}),
    "realT_imagT": (E43, C5, CRI, dict(mul_args=RI)),
    "realT_loose": (E43, C5, CC, dict(mul_args=RealComplexMul(realT=Tags(9, 2, QuMode=RND.CONV), loose=Tags(OfMode=SAT.ZERO)))),
    "two_types_e88": (E88, C88, CC, dict(mul_args=QQ)),
    "two_types": (E43, C5, CC, dict(mul_args=QQ)),
    "levels_tags": (E43, C5, CC, dict(mul_args=RI, add_args=L12)),
    "levels": (E43, C5, CC, dict(add_args=L12)),
    "exact_e88": (E88, C88, Qcomplex(Qu(28, 10), Qu(27, 13)), dict(mul_args=RealComplexMul(realT=Qu(17, 16), imagT=Qu(16, 13)), add_args=[Qcomplex(Qu(28, 16), Qu(27, 13))])),
    "exact": (E43, C5, CWD, dict(mul_args=RealComplexMul(realT=Qu(12, 6), imagT=Qu(12, 3)), add_args=[Qcomplex(Qu(24, 6), Qu(24, 3))])),
    "level70": (E43, C5, CWD, dict(add_args=[Qcomplex(Qu(40, 30), Qu(12, 3))])),
}


def lowered(j):
    key = next(k for k in TAGS if j["name"].startswith(k + "_"))   # (dict order: the longer prefix of a pair comes first)
    er, ez, ec, kw = TAGS[key]
    ea, eb = (er, ez) if j["name"].endswith("_ra") else (ez, er)
    return lower(ea, eb, ec, j["M"], j["N"], j["K"], transposed_a=bool(j["transA"]), **kw)


@pytest.mark.parametrize("j", CASES, ids=lambda j: j["name"])
def test_checker_equals_the_reference(j):
    d, A, B, got = R.case_checked(j["name"])
    assert got.tobytes() == R.case_expected(j).tobytes()
    assert R.strong(d, got) or "saturation" in j["name"]


def test_golden_set_covers_what_it_should():
    names = [j["name"] for j in CASES]
    assert len(names) == len(set(names)) and sum(n.endswith("_ra") for n in names) == sum(n.endswith("_rb") for n in names) == len(names) // 2
    assert {j["K"] for j in CASES} >= {1, 2, 5, 37, 64, 1000}
    assert {j["inputs"]["dist"] for j in CASES} == {0, 2} and any(j["transA"] for j in CASES)
    assert {j["cmul"] for j in CASES} == {CMUL_REAL_A, CMUL_REAL_B}
    for j in CASES:   # the real operand has one spelling
        assert (j["a"] if j["cmul"] == CMUL_REAL_A else j["b"])[1] == [0, 0, 0, 0, 0]
    by = {j["name"]: j for j in CASES}
    assert by["default_9x7xK37_full_ra"]["mul"][:2] == [[6, 3, 1, 5, 0], [6, 3, 1, 5, 0]]             # both parts land in (6, 3)
    assert by["realT_imagT_9x7xK37_edges_rb"]["mul"][:2] == [[12, 6, 1, 5, 0], [10, 0, 1, 5, 0]]       # exactly the tagged formats


@pytest.mark.parametrize("j", CASES, ids=lambda j: j["name"])
def test_python_lowering_reproduces_the_reference_formats(j):
    got, want = desc_to_dict(lowered(j)), desc_to_dict(R.case_desc(j))
    assert got == want


def test_standalone_header_lowering(tmp_path):
    """include/QuBLAS_amd.h lowers the same tags to the same descriptors, byte for byte with the Python lowering and the reference's types"""
    import json
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("needs AMD clang (C++23)")
    exe = str(tmp_path / "mixed_probe")
    subprocess.check_call([clang, "-std=c++23", "-O0", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "binding"),
                           os.path.join(ROOT, "tests", "binding", "amd_header_mixed_probe.cpp"), "-o", exe])
    recs = [json.loads(l) for l in subprocess.check_output([exe], text=True).splitlines() if l.strip()]
    gold = {j["name"]: j for j in CASES}
    assert len(recs) == len(CASES) == 36 and {r["cmul"] for r in recs} == {CMUL_REAL_A, CMUL_REAL_B}
    for r in recs:
        want = desc_to_dict(R.case_desc(gold[r["name"]]))
        for k in ("M", "N", "K", "transA", "is_complex", "cmul", "a", "b", "c", "mul", "n_levels", "level_add", "level"):
            assert r[k] == want[k], (r["name"], k)
        assert desc_to_dict(lowered(gold[r["name"]])) == want


def _reference_include():
    """the reference's include directory: REF_INC of the environment, else the default of oracle/Makefile; None where it is absent"""
    inc = os.environ.get("REF_INC")
    if not inc:
        m = re.search(r"^REF_INC \?= (\S+)", open(os.path.join(ROOT, "oracle", "Makefile")).read(), re.M)
        inc = m.group(1) if m else None
    return inc if inc and os.path.exists(os.path.join(inc, "QuBLAS.h")) else None


@pytest.mark.skipif(_reference_include() is None, reason="the reference header is not on this machine (it cannot travel)")
def test_reference_binding_lowering(tmp_path):
    """include/qgemul_reference_binding.hpp on the reference's own types (decltype of its own Qmul): the same descriptors"""
    import json
    exe = str(tmp_path / "ref_mixed_probe")
    subprocess.check_call(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++23", "-O0", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "binding"),
                           "-I" + _reference_include(), os.path.join(ROOT, "tests", "binding", "ref_binding_mixed_probe.cpp"), "-o", exe])
    recs = [json.loads(l) for l in subprocess.check_output([exe], text=True).splitlines() if l.strip()]
    gold = {j["name"]: j for j in CASES}
    assert len(recs) == len(CASES) == 36
    for r in recs:
        want = desc_to_dict(R.case_desc(gold[r["name"]]))
        for k in ("M", "N", "K", "transA", "is_complex", "cmul", "a", "b", "c", "mul", "n_levels", "level_add", "level"):
            assert r[k] == want[k], (r["name"], k)


def test_lowering_refuses_what_is_no_mixed_call():
    with pytest.raises(ValueError):
        lower(E43, C5, E43, 4, 4, 4)            # a real C
    with pytest.raises(ValueError):
        lower(E43, C5, CC, 4, 4, 4, mul_args=object())
    with pytest.raises(ValueError):
        lower(E43, C5, CC, 4, 4, 4, add_args=[Qu(9, 3)])   # real level types on a complex tree


def test_classify_answers_a_mixed_descriptor():
    """fails on a library without the feature: QG_EINVAL, "complex descriptor without cmul\""""
    M, N, K = 100, 70, 300
    for order, cmul in (("ra", CMUL_REAL_A), ("rb", CMUL_REAL_B)):
        ea, eb = (E43, C5) if order == "ra" else (C5, E43)
        d = lower(ea, eb, CC, M, N, K)
        assert d.cmul == cmul and d.is_complex == 1
        st, info = capi.classify_status(d)
        assert st == capi.QG_OK and info.supported == 1 and info.cls == CLASS_TREE
        assert capi.KERNEL_NAMES[info.kernel] == "tree_rc_i32"
        reason = info.reason.decode()
        assert reason.startswith("real x complex" if order == "ra" else "complex x real") and reason.endswith("fixed modes, compact")
        assert info.ops == 4.0 * M * N * K
        real, cplx = (0, 1) if order == "ra" else (1, 0)
        assert info.host_elem_bytes[real] == 4 and info.host_imag_off[real] == 0          # a plain word
        assert info.host_elem_bytes[cplx] == 8 and info.host_imag_off[cplx] == 4          # struct {real; imag;}
        assert info.host_elem_bytes[2] == 8 and info.host_imag_off[2] == 4
        Kp = 512                                                                           # 9 levels: zero-padded to 2^9 leaves
        assert info.packed_bytes[real] == (M if order == "ra" else N) * Kp * 4             # [rows][K]
        assert info.packed_bytes[cplx] == 2 * (N if order == "ra" else M) * Kp * 4         # [2][rows][K]
        assert info.packed_bytes[2] == 2 * M * N * 4                                       # what a complex plan of the class produces
        # the flags act as on complex plans
        i2 = capi.classify(d, capi.OPT_RUNTIME_MODES)
        assert capi.KERNEL_NAMES[i2.kernel] == "tree_rc_i32" and i2.reason.decode().endswith("run-time modes")
        i3 = capi.classify(d, capi.OPT_GENERIC_TREE)
        assert capi.KERNEL_NAMES[i3.kernel] == "tree_cplx" and i3.packed_bytes[real] == (M if order == "ra" else N) * K * 4
        assert capi.classify(d, capi.OPT_FORCE_TREE).kernel == info.kernel
        # a wide real operand: an 8-byte word
        dw = lower(*((Qu(20, 20), C5) if order == "ra" else (C5, Qu(20, 20))), Qcomplex(Qu(30, 20), Qu(30, 20)), 8, 8, 8)
        iw = capi.classify(dw)
        assert iw.host_elem_bytes[real] == 8 and iw.host_imag_off[real] == 0 and capi.KERNEL_NAMES[iw.kernel] == "tree_cplx"


def test_step_forms_and_kernels():
    kinds = lower(E43, C5, CC, 33, 17, 100, mul_args=QQ, add_args=L12)      # value-dependent roundings, wrapping: no compact form
    assert capi.classify(kinds).reason.decode().endswith("mixed kernel steps: run-time modes")
    long_rt = lower(E43, C5, CC, 4, 4, 8192, mul_args=QQ, add_args=L12)     # 13 levels: the run-time form is built for 12
    assert capi.KERNEL_NAMES[capi.classify(long_rt).kernel] == "tree_cplx"
    long_c = lower(E43, C5, CC, 4, 4, 8192)
    assert capi.KERNEL_NAMES[capi.classify(long_c).kernel] == "tree_rc_i32"
    assert capi.KERNEL_NAMES[capi.classify(long_c, capi.OPT_RUNTIME_MODES).kernel] == "tree_cplx"
    wide = lower(E43, C5, CWD, 9, 7, 37, add_args=[Qcomplex(Qu(40, 30), Qu(12, 3))])
    info = capi.classify(wide)
    assert capi.KERNEL_NAMES[info.kernel] == "tree_i128" and "real x complex" in info.reason.decode()
    # exact products and levels: the linear class, one real limb GEMM on the stacked operand + the two-product convert pass
    for order in ("ra", "rb"):
        ea, eb = (E43, C5) if order == "ra" else (C5, E43)
        exact = lower(ea, eb, CWD, 130, 70, 200, mul_args=RealComplexMul(realT=Qu(12, 6), imagT=Qu(12, 3)), add_args=[Qcomplex(Qu(24, 6), Qu(24, 3))])
        info = capi.classify(exact)
        assert info.cls == CLASS_LINEAR and capi.KERNEL_NAMES[info.kernel] == "mfma_rc" and list(info.limbs) == ([1, 2] if order == "ra" else [2, 1])
        reason = info.reason.decode()
        assert reason.startswith("real x complex: linear class" if order == "ra" else "complex x real: linear class") and "two-product convert" in reason
        assert info.ops == 4.0 * 130 * 70 * 200 and info.packed_bytes[2] == 2 * 130 * 70 * 4
        real, cplx = (0, 1) if order == "ra" else (1, 0)
        assert info.packed_bytes[cplx] > info.packed_bytes[real]          # the complex operand's parts are stacked along its rows
        forced = capi.classify(exact, capi.OPT_FORCE_TREE)                # ... and QG_OPT_FORCE_TREE selects the tree plan
        assert capi.KERNEL_NAMES[forced.kernel] == "tree_rc_i32" and forced.limbs[0] == 0
        # a product that can round keeps the tree class; K beyond the int32 accumulators' exact range goes to the tree kernels
        assert capi.classify(lower(ea, eb, CWD, 130, 70, 200, mul_args=RealComplexMul(realT=Qu(12, 5), imagT=Qu(12, 3)))).cls == CLASS_TREE
        long_k = lower(ea, eb, Qcomplex(Qu(30, 6), Qu(30, 3)), 8, 8, 1 << 17, mul_args=RealComplexMul(realT=Qu(12, 6), imagT=Qu(12, 3)), add_args=[Qcomplex(Qu(30, 6), Qu(30, 3))])
        assert capi.KERNEL_NAMES[capi.classify(long_k).kernel] in ("tree_cplx", "tree_rc_i32")


def test_malformed_mixed_descriptors_are_einval():
    d = lower(E43, C5, CC, 8, 8, 8)
    st, info = capi.classify_status(d)
    assert st == capi.QG_OK
    bad = lower(E43, C5, CC, 8, 8, 8)
    bad.a[1] = Qu(4, 3).c()                     # the real operand's [1] must be all zero
    st, info = capi.classify_status(bad)
    assert st == capi.QG_EINVAL and "must be zero" in info.reason.decode()
    bad = lower(C5, E43, CC, 8, 8, 8)
    bad.b[1].O = 1
    assert capi.classify_status(bad)[0] == capi.QG_EINVAL
    padded = lower(C5, E43, CC, 8, 8, 8)
    padded.b[1].pad = 0x5a                      # padding bytes are no part of a format's meaning
    assert capi.classify_status(padded)[0] == capi.QG_OK
    bad = lower(E43, C5, CC, 8, 8, 8)
    bad.is_complex = 0                          # C of a mixed product is complex
    assert capi.classify_status(bad)[0] == capi.QG_EINVAL
    bad = lower(E43, C5, CC, 8, 8, 8)
    bad.cmul = 5                                # no such multiplier
    st, info = capi.classify_status(bad)
    assert st == capi.QG_EINVAL and "without cmul" in info.reason.decode()
    bad = lower(E43, C5, CC, 8, 8, 8)
    bad.n_levels = 2
    assert capi.classify_status(bad)[0] == capi.QG_EINVAL
    bad = lower(E43, C5, CC, 8, 8, 8)
    bad.mul[1].Q = 9                            # a product slot with an unknown mode
    assert capi.classify_status(bad)[0] == capi.QG_EINVAL
    # the refusal rules act per part: an operand element beyond 64 storage bits
    big = lower(Qu(40, 30), C5, Qcomplex(Qu(50, 30), Qu(50, 30)), 8, 8, 8)
    assert capi.classify_status(big)[0] == capi.QG_EUNSUPPORTED


def test_refusals_say_mixed_real_complex():
    for d in (lower(E43, C5, CC, 16, 16, 16), lower(C5, E43, CC, 16, 16, 16)):
        ep = qgemul_epilogue()
        ep.d = d.c[0]
        st, info = capi.classify_ep_status(d, ep)
        assert st == capi.QG_EUNSUPPORTED and "mixed real-complex" in info.reason.decode() and info.supported == 0
        epc = qgemul_epilogue_cplx()
        epc.part[0].d, epc.part[1].d = d.c[0], d.c[1]
        st, info = capi.classify_ep_status(d, epc)
        assert st == capi.QG_EUNSUPPORTED and "mixed real-complex" in info.reason.decode()
        st, info = capi.classify_epcx(d, epc, [])
        assert st == capi.QG_EUNSUPPORTED and "mixed real-complex" in info.reason.decode()
        st, info = capi.classify_batched_status(d, 3)
        assert st == capi.QG_EUNSUPPORTED and "mixed real-complex" in info.reason.decode()
        st, info = capi.classify_grouped_status([d, d])
        assert st == capi.QG_EUNSUPPORTED and "mixed real-complex" in info.reason.decode()
        # the sharded run: refused before any device is touched
        ea, eb, ec = R.elems(d)
        from oracle import qoracle
        A, B = qoracle.fill(ea, 16 * 16, 1), qoracle.fill(eb, 16 * 16, 2)
        out = np.zeros(16 * 16, dtype=qoracle.host_dtype(ec))
        L = capi.lib()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        devs = (C.c_int * 1)(0)
        assert L.qgemul_run_sharded(C.byref(d), p(out), p(A), p(B), None, devs, 1) == capi.QG_EUNSUPPORTED
        from qublas_amd.desc import qgemul_opts
        o = qgemul_opts(0, 0, 0, -1, capi.OPT_ALL_DEVICES)
        assert L.qgemul_run(C.byref(d), p(out), p(A), p(B), C.byref(o)) == capi.QG_EUNSUPPORTED


# ---- the planner under sanitizers, as a stand-alone program ----
def random_mixed(n, seed):
    """random mixed descriptors: formats, tags, level lists, shapes; a third damaged on purpose"""
    rng = random.Random(seed)
    out = []

    def qu(maxw):
        w = rng.randint(1, maxw)
        f = rng.randint(-3, w + 2)
        return Qu(w - f, f, rng.random() < 0.8, rng.randint(0, 6), rng.randint(0, 3))
    while len(out) < n:
        er, ez = qu(rng.choice([8, 14, 30])), Qcomplex(qu(14), qu(14))
        ec = Qcomplex(qu(40), qu(40))
        kw = {}
        if rng.random() < 0.6:
            kw["mul_args"] = RealComplexMul(realT=qu(30) if rng.random() < 0.7 else None, imagT=qu(30) if rng.random() < 0.7 else None,
                                            loose=Tags(FullPrec=True) if rng.random() < 0.3 else None)
        if rng.random() < 0.6:
            kw["add_args"] = [Qcomplex(qu(rng.choice([20, 40, 70])), qu(40)) for _ in range(rng.randint(1, 3))]
        M, N, K = rng.randint(0, 300), rng.randint(0, 300), rng.choice([1, 2, 5, 31, 32, 33, 1000, 5000, 70000])
        ea, eb = (er, ez) if rng.random() < 0.5 else (ez, er)
        d = lower(ea, eb, ec, M, N, K, transposed_a=rng.random() < 0.3, **kw)
        hit = rng.random()
        if hit < 0.08:
            (d.a if d.cmul == CMUL_REAL_A else d.b)[1].F = 3
        elif hit < 0.14:
            d.is_complex = 0
        elif hit < 0.2:
            d.cmul = rng.choice([0, 5, 200])
        elif hit < 0.26:
            d.mul[rng.randint(0, 1)].O = 7
        elif hit < 0.3:
            d.n_levels = rng.randint(0, 41)
        elif hit < 0.33:
            d.cmul = CMUL_REAL_A if d.cmul == CMUL_REAL_B else CMUL_REAL_B   # the other order's spelling on this one's formats
        out.append(d)
    return out


def exact_mixed(n, seed):
    """mixed descriptors whose products and levels hold every value: the linear class, one to three limbs per operand"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        wr, wz = rng.choice([6, 12, 17, 20]), rng.choice([6, 12, 17])
        er = Qu(wr - 3, 3)
        ez = Qcomplex(Qu(wz - 2, 2), Qu(wz - 4, 4))
        M, N, K = rng.randint(1, 200), rng.randint(1, 200), rng.choice([1, 7, 40, 200, 3000])
        lg = max(1, (K - 1).bit_length())
        pr, pi = Qu(er.intBits + ez.real.intBits + 2, 5), Qu(er.intBits + ez.imag.intBits + 2, 7)
        lv = Qcomplex(Qu(pr.intBits + lg, 5), Qu(pi.intBits + lg, 7))
        ea, eb = (er, ez) if rng.random() < 0.5 else (ez, er)
        out.append(lower(ea, eb, lv, M, N, K, transposed_a=rng.random() < 0.3, mul_args=RealComplexMul(realT=pr, imagT=pi), add_args=[lv]))
    return out


def test_the_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mixed_plan_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "mixed_plan_san_driver.cpp"), os.path.join(CSRC, "qg_geom.cpp"), os.path.join(CSRC, "qg_plan.cpp"), "-o", exe])
    descs = [R.case_desc(j) for j in CASES] + random_mixed(1500, 5) + exact_mixed(40, 6)
    flags = [0, capi.OPT_FORCE_TREE, capi.OPT_GENERIC_TREE, capi.OPT_RUNTIME_MODES]
    queries = [(flags[i % 4], (0, 0, 0, 1, 2)[i % 5], d) for i, d in enumerate(descs)]
    wire = b"".join(struct.pack("<II", f, k) + bytes(d) for f, k, d in queries)
    r = subprocess.run([exe], input=wire, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"ERROR" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(queries)
    seen = {}
    for (f, k, d), line in zip(queries, lines):
        if k == 0:
            st, i = capi.classify_status(d, f)
        elif k == 1:
            st, i = capi.classify_batched_status(d, 3, f)
        else:
            ep = qgemul_epilogue()
            ep.d = d.c[0]
            st, i = capi.classify_ep_status(d, ep, f)
        ok = st == capi.QG_OK
        z = lambda v: v if ok else 0
        want = "st=%d sup=%d cls=%d kernel=%d max_bits=%d in_bits=%d,%d packed=%d,%d,%d ops=%s heb=%d,%d,%d hio=%d,%d,%d reason=%s" % (
            st, i.supported, z(i.cls), z(i.kernel), z(i.max_bits), z(i.in_bits[0]), z(i.in_bits[1]), z(i.packed_bytes[0]), z(i.packed_bytes[1]), z(i.packed_bytes[2]),
            "%.17g" % (i.ops if ok else 0.0), z(i.host_elem_bytes[0]), z(i.host_elem_bytes[1]), z(i.host_elem_bytes[2]), z(i.host_imag_off[0]), z(i.host_imag_off[1]),
            z(i.host_imag_off[2]), i.reason.decode())
        assert line == want, (line, want)
        key = (st, capi.KERNEL_NAMES.get(i.kernel) if ok else None)
        seen[key] = seen.get(key, 0) + 1
    # every answer is exercised
    for key in ((capi.QG_OK, "tree_rc_i32"), (capi.QG_OK, "tree_cplx"), (capi.QG_OK, "tree_i128"), (capi.QG_EINVAL, None), (capi.QG_EUNSUPPORTED, None)):
        assert seen.get(key, 0) >= 10, (key, seen)
    assert seen.get((capi.QG_OK, "mfma_rc"), 0) >= 4, seen   # the linear class: the exact golden records and the exact random ones


# ---- the compiler's resource report of the mixed tree kernel ----
def parse_resources(text):
    kernels, cur = {}, None
    for ln in text.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z /\[\]]+?): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def check_resources(kernels):
    rc = {k: v for k, v in kernels.items() if "k_tree_rc" in k}
    assert len(rc) == 6, sorted(rc)     # compact: 12 and 16 levels, run-time: 12 levels; each for both operand orders
    for name, v in rc.items():
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (name, v)
        assert v["LDS Size [bytes/block]"] == 3 * 32 * 36 * 4, (name, v)   # one plane of the real operand, two of the complex one


def test_committed_resource_report_has_no_scratch():
    check_resources(parse_resources(open(os.path.join(ROOT, "profiles", "mixed_kernel_resources.txt")).read()))


def test_mixed_kernel_uses_no_scratch(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("needs hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", os.path.join(CSRC, "qg_tree_rc.hip"), "-o",
                        str(tmp_path / "rc.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    check_resources(parse_resources(r.stderr))
