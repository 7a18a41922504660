"""Every byte qg_analyze, qg_analyze_epx and qg_analyze_epcx write, as a digest (tests/san/plan_san_driver.cpp --digest): the planner is
host-only and deterministic, so two builds of it that print the same digests over one corpus wrote the same tables.  This test pins
what makes such a comparison mean something — the plain build and the build under AddressSanitizer + UndefinedBehaviorSanitizer
agree line for line (no byte of an output depends on uninitialised memory or on the optimiser), nothing is reported, and the corpus
reaches every step form and every branch of the analysis named below.  It stores no hash: tools/plan_digest.py compares two
revisions of qublas_amd/csrc/qg_plan.cpp over the same corpus."""
import os
import struct
import subprocess

import geom_sweep as S
import golden_io as G
import mixed_ref
import test_mixed_plan as TM
import test_ring_plan as TR
from test_plan_sanitizers import compact_form_descs, random_descs
from qublas_amd import capi
from qublas_amd.desc import DESC_LEFTOVER0_COPY, Qu, SAT, TRN, WRP, Tags, desc_from_dict, lower

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
DRIVER = os.path.join(ROOT, "tests", "san", "plan_san_driver.cpp")
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]


def hand_written():
    """the branches of the analysis no other corpus reaches"""
    e88 = Qu(8, 8)
    out = []
    # QG_DESC_LEFTOVER0_COPY with an odd K: only the general kernel may run it
    d = lower(e88, e88, Qu(24, 8), 9, 7, 101, mul_args=Tags(17, 16), add_args=[Qu(29, 16, True, TRN.TCPL, SAT.ZERO)])
    d.flags |= DESC_LEFTOVER0_COPY
    out.append(d)
    # QG_DESC_REFERENCE_ARTEFACTS on a C of an unsigned WRP::TCPL format with exactly 32 value bits: analysed as WRP::TCPL_SAT
    out.append(lower(e88, e88, Qu(24, 8, False, TRN.TCPL, WRP.TCPL), 9, 7, 64, reference_artefacts=True))
    return out


def corpus():
    """[(descriptor, None | ("epx", epilogue, tables) | ("epcx", complex epilogue, CMUL records))]"""
    descs = [desc_from_dict(j) for j in G.gemm_cases("real") + G.gemm_cases("cplx")] + random_descs(3000, 5) + compact_form_descs(1500, 6)
    descs += S.descriptors(500, 250)
    descs += [mixed_ref.case_desc(j) for j in TM.CASES] + TM.random_mixed(1500, 5) + TM.exact_mixed(40, 6)
    descs += [r[1] for r in TR.RINGS] + [r[1] for r in TR.NEIGHBOURS] + hand_written()
    out = [(d, None) for d in descs]
    out += [(d, ("epx", ep, tabs)) for d, ep, tabs, _ in S.real_chains()]
    out += [(d, ("epcx", epc, cx)) for d, epc, cx in S.cplx_chains()]
    return out


def wire(records) -> bytes:
    out = bytearray()
    for d, chain in records:
        out += struct.pack("<I", S.CHAIN_KIND[chain[0]] if chain else 0) + bytes(d)
        if chain:
            recs = (list(chain[2]) + [None] * capi.QG_MAX_EW)[:capi.QG_MAX_EW]
            out += bytes(chain[1]) + bytes(1 if r is not None else 0 for r in recs) + b"".join(bytes(r) for r in recs if r is not None)
    return bytes(out)


def start_build(exe, flags, plan_cpp=os.path.join(CSRC, "qg_plan.cpp")):
    return subprocess.Popen(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, DRIVER, plan_cpp, "-o", exe])


def build_driver(exe, flags, plan_cpp=os.path.join(CSRC, "qg_plan.cpp")):
    assert start_build(exe, flags, plan_cpp).wait() == 0
    return exe


def parse_counts(line):
    """{name: count} of a "name=count" line, {form: count} of a "form:count" line"""
    toks = line.split()[1:]
    return {k: int(v) for k, v in (t.split("=") for t in toks)} if "=" in line else {int(k): int(v) for k, v in (t.split(":") for t in toks)}


def test_digest_is_deterministic_and_the_corpus_reaches_every_form(tmp_path):
    plain, san = str(tmp_path / "plan_digest"), str(tmp_path / "plan_digest_san")
    builds = [start_build(plain, ["-O2"]), start_build(san, SANITIZE)]   # (both compile while the corpus is made)
    records = corpus()
    blob = wire(records)
    assert [b.wait() for b in builds] == [0, 0]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    runs = [subprocess.run([exe, "--digest"], input=blob, capture_output=True, env=env, timeout=300) for exe in (plain, san)]
    for r in runs:
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr and b"LeakSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    assert runs[0].stdout == runs[1].stdout
    lines = runs[0].stdout.decode().splitlines()
    assert len(lines) == len(records) + 6 and lines[-1].split()[:2] == ["digest", str(len(records))], lines[-6:]
    print("\n".join(lines[-6:]))
    status, tree, gemv, cplx, covered = (parse_counts(ln) for ln in lines[-6:-1])
    assert lines[-6].startswith("status ") and lines[-2].startswith("covered ")
    assert all(status[k] > 0 for k in ("ok", "einval", "eunsupported")), status
    # every enumerator of QTreeForm, QGemvForm and QCplxForm (qublas_amd/csrc/qg_forms.h) is the analysed form of an accepted descriptor
    assert set(tree) == set(range(0, 10)) | set(range(16, 25)), sorted(tree)
    assert set(gemv) == {0, 1, 2, 3, 5, 6, 7}, sorted(gemv)
    assert set(cplx) == set(range(0, 7)) | set(range(9, 14)) | {15}, sorted(cplx)
    for k in ("wide", "band", "generic_only", "ring_ok", "real_a", "real_b", "cmul_tf", "cmul_basic", "leftover0_copy_odd_k", "artefact_rewrites_c", "split_s",
              "biased_fallback", "uniform_basic", "real_chains", "cplx_chains"):
        assert covered[k] > 0, (k, covered)
    # a record's digest covers its status too: the distinct digests are at least the accepted descriptors' distinct plans
    assert len({ln.split(" ", 1)[1] for ln in lines[:-6]}) > 1000


def test_forms_header_names_no_form_the_test_does_not():
    """the sets above are qg_forms.h's enumerators: a new form must be added to the corpus and to this test"""
    import re
    text = open(os.path.join(CSRC, "qg_forms.h")).read()
    values = {p: {int(v) for v in re.findall(p + r"_\w+ = (\d+)", text)} for p in ("QTF", "QGF", "QCF")}
    assert values["QTF"] == set(range(0, 10)) | set(range(16, 25))
    assert values["QGF"] == {0, 1, 2, 3, 5, 6, 7}
    assert values["QCF"] == set(range(0, 7)) | set(range(9, 14)) | {15}
