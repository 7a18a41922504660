"""Coverage guard: every step form of the 32-bit tree kernels (qublas_amd/csrc/qg_forms.h: QTreeForm, QGemvForm, QCplxForm) and
every linear plan kind is reached by at least one GEMM record that the REAL reference produced at the edge-heavy operand
distribution (dist 2: tests/golden/ref_gemm_*.jsonl.gz, oracle/ref_cases_*.cpp), and by one with K <= 3 (the product step alone,
one node).  A form added later without such a reference vector fails here.  The forms are read through the planner driver
(tests/san/plan_san_driver.cpp, built without sanitizers), not from reason strings, which merge several forms.  CPU only."""
import os
import re
import subprocess

import pytest

import golden_io as G
from qublas_amd import capi
from qublas_amd.desc import desc_from_dict, lower, qgemul_epilogue

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the run-time-mode forms: no plan takes them by default.  Every dist-2 record runs under QG_OPT_RUNTIME_MODES in
# tests/test_gpu_edges.py::test_edge_records_second_opinions; the flag sends 32-bit words to the 64-bit kernels and every other
# plan of these three kernels to the form below, which test_run_time_forms_are_reached_under_the_flag checks
EXCLUDED = {
    "QTF_RUNTIME": "tree_i32",
    "QGF_RUNTIME": "gemv_i32",
    "QCF_RUNTIME": "tree_cplx_i32",
}
# the planner picks these only for rows of at least 256 leaves (qg_plan.cpp: gemv_w32 with n_levels_k >= 8): no K <= 3 record
LONG_ROWS = {"QGF_WORD", "QGF_WORD_RND"}


def enumerators():
    src = open(os.path.join(ROOT, "qublas_amd", "csrc", "qg_forms.h")).read()
    out = {}
    for enum in ("QTreeForm", "QGemvForm", "QCplxForm"):
        body = re.search(r"enum %s : int \{(.*?)\};" % enum, src, re.S).group(1)
        out[enum] = {int(v): n for n, v in re.findall(r"^\s*(Q\w+)\s*=\s*(\d+)", body, re.M)}
        assert out[enum], enum
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join(ROOT, "tests", "san", "plan_san_driver.cpp"),
                           os.path.join(ROOT, "qublas_amd", "csrc", "qg_plan.cpp"), "-o", exe])
    return exe


def driver_lines(exe, descs):
    blob = b"".join(bytes(d) + bytes(qgemul_epilogue()) for d in descs)
    r = subprocess.run([exe], input=blob, capture_output=True, check=True, timeout=300)
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(descs)
    return lines


def forms_of(exe, descs):
    """the step form each descriptor's plan runs (enumerator name), or None where no 32-bit tree kernel runs it"""
    names = enumerators()
    lines = driver_lines(exe, descs)
    out = []
    kernel_enum = {"tree_i32": ("QTreeForm", 7), "gemv_i32": ("QGemvForm", 9), "tree_cplx_i32": ("QCplxForm", 8)}
    for ln, d in zip(lines, descs):
        head, plain, _, _ = ln.split("|")
        f = head.split()
        kernel = capi.KERNEL_NAMES[capi.classify(d).kernel] if int(f[1]) == 0 else "none"   # (the plan the product library runs)
        if kernel in kernel_enum:
            assert capi.KERNEL_NAMES[int(plain.split()[0])] == kernel, ln
            enum, col = kernel_enum[kernel]
            out.append(names[enum][int(f[col])])
        else:
            out.append(None)
    return out


def linear_kind(d):
    """single-limb, plain limbs, or centred NxN (limbs fewer than under QG_OPT_BALANCED_LIMBS) for the MFMA plans"""
    info = capi.classify(d)
    if capi.KERNEL_NAMES[info.kernel] not in ("mfma_i8", "mfma_i8_limb"):
        return None
    limbs, bal = list(info.limbs), list(capi.classify(d, capi.OPT_BALANCED_LIMBS).limbs)
    if limbs != bal:
        return "centred %dx%d" % tuple(limbs)
    return "single-limb" if limbs == [1, 1] else "plain limbs"


def records():
    return G.gemm_cases("real") + G.gemm_cases("cplx")


def dist(j):
    """the generator distribution of a record's operands (seeded, or explicit values drawn from seeds)"""
    return j["inputs"].get("dist", j["inputs"].get("from", {}).get("dist"))


def test_every_step_form_has_an_edge_reference_vector(driver):
    recs = records()
    fm = forms_of(driver, [desc_from_dict(j) for j in recs])
    edge = {f for j, f in zip(recs, fm) if dist(j) == 2}
    short = {f for j, f in zip(recs, fm) if dist(j) == 2 and j["K"] <= 3}
    for enum, vals in enumerators().items():
        for name in vals.values():
            if name in EXCLUDED:
                continue
            assert name in edge, f"{enum}::{name}: no reference record at dist 2 reaches it (oracle/ref_cases_*.cpp)"
            if name not in LONG_ROWS:
                assert name in short, f"{enum}::{name}: no reference record with K <= 3 reaches it"


def test_every_linear_plan_kind_has_an_edge_reference_vector():
    need = {"single-limb", "plain limbs", "centred 1x1", "centred 2x2", "centred 3x3"}
    edge, short = set(), set()
    for j in records():
        if j["is_complex"]:
            continue
        k = linear_kind(desc_from_dict(j))
        if dist(j) == 2:
            edge.add(k)
            if j["K"] <= 3:
                short.add(k)
    assert need <= edge, need - edge
    assert need <= short, need - short


def test_exclusions_are_enumerators():
    names = {n for vals in enumerators().values() for n in vals.values()}
    assert set(EXCLUDED) <= names and LONG_ROWS <= names


def test_run_time_forms_are_reached_under_the_flag(driver):
    """the excluded run-time-mode forms: dist-2 records reach each of the three kernels under QG_OPT_RUNTIME_MODES with
    their run-time-mode steps (the planner driver's second column of kernel choices)"""
    recs = [j for j in records() if dist(j) == 2]
    descs = [desc_from_dict(j) for j in recs]
    seen = set()
    for ln, d in zip(driver_lines(driver, descs), descs):
        kernel, name = ln.split("|")[2].split(" ", 1)
        if int(kernel) > 0 and capi.classify(d, capi.OPT_RUNTIME_MODES).kernel == int(kernel) and name == "run-time modes":
            seen.add(capi.KERNEL_NAMES[int(kernel)])
    assert set(EXCLUDED.values()) <= seen, seen


def test_gpu_edge_cases_reach_their_forms(driver):
    """tests/test_gpu_edges.py names the step form each of its cases runs: every case reaches it at every shape it runs"""
    import test_gpu_edges as E
    descs, want = [], []
    for ea, eb, ec, kw, _, _, form in E.REAL:
        for M, N, K in E.SHAPES:
            descs.append(lower(ea, eb, ec, M, N, K, transposed_a=K == 513, **kw))
            want.append(form)
    for e, levels, shapes, _, gemv_form, reduce_form in E.COLUMN:
        for rows, K in shapes:
            (g, _, _), (r, _, _) = E.column_cases(e, levels, rows, K, None)
            descs += [g, r]
            want += [gemv_form, reduce_form]
    for e, ec, kw, form in E.CPLX:
        for M, N, K in E.SHAPES:
            descs.append(lower(e, e, ec, M, N, K, transposed_a=K == 513, **kw))
            want.append(form)
    got = forms_of(driver, descs)
    bad = [(i, w, g) for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not bad, bad
    names = {n for vals in enumerators().values() for n in vals.values()}
    assert names - set(EXCLUDED) - {w for w in want if w} == set(), "a step form without a case in tests/test_gpu_edges.py"
