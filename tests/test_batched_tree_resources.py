"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of the batched twins of the tiled 32-bit tree kernels
(QG_OPT_BATCHED_TREE; qublas_amd/csrc/qg_tree_fast_bd.hip, qg_tree_cplx_bd.hip: the text of k_tree_fast, k_tree_pk16, k_tree_cplx and
k_tree_cplx_pk16 compiled again behind the walk over the members, at MAXL == 12).  Every twin is compared with its plain kernel from a compile of the
same tree (qg_tree_fast.hip, qg_tree_cplx.hip): no more scratch, no more spilled vector registers, no more spilled scalar registers,
no lower occupancy, and 16 bytes of LDS more (the member's C and the container size).  Every figure of the fresh compile of the two
new units equals the committed report profiles/batched_tree_kernel_resources.txt.  hipcc cross-compiles for gfx950 without a GPU: CPU
only; the four units compile side by side."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNITS = {"qg_tree_fast_bd.hip": "qg_tree_fast.hip", "qg_tree_cplx_bd.hip": "qg_tree_cplx.hip"}   # the twins' unit -> the plain kernels'
# instantiations: k_tree_fast 5 word forms + 2 left-justified + 2 x 7 with and without a split product, k_tree_pk16 3 x 2,
# k_tree_cplx 12 forms x 2 multipliers, k_tree_cplx_pk16 2
COUNT = {"k_tree_fast": 21, "k_tree_pk16": 6, "k_tree_cplx": 24, "k_tree_cplx_pk16": 2}
MEMBER_WORDS = 2 * 8   # C of the member and the container size, which wait in LDS while the k-loop runs (qg_tree_bd.h)


def parse(text):
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


def key(symbol):
    """(kernel, template arguments) of a mangled kernel name, the twin's "_bd" dropped; None: no tiled tree kernel"""
    m = re.search(r"\d+(k_tree_(?:fast|pk16|cplx|cplx_pk16))(_bd)?I(.*?)EEvNS", symbol)
    return (m.group(1), m.group(3), bool(m.group(2))) if m else None


def maxl(k):
    """the MAXL template argument of a key: the third of k_tree_fast, the first of the others"""
    args = re.findall(r"L[ib](\d+)E", k[1])
    return int(args[2 if k[0] == "k_tree_fast" else 0])


def committed():
    """the committed report: the remarks of one kernel on one line, "Function Name: <symbol>; <figure>: <n>; ..." """
    kernels = {}
    for ln in open(os.path.join(ROOT, "profiles", "batched_tree_kernel_resources.txt")):
        if ln.startswith("Function Name: "):
            name, *figs = ln.strip().split("; ")
            kernels[name.split(": ")[1]] = {k: int(v) for k, v in (f.rsplit(": ", 1) for f in figs) if v.isdigit()}
    return kernels


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    tmp = tmp_path_factory.mktemp("batched_tree")
    srcs = sorted(set(UNITS) | set(UNITS.values()))
    procs = [subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-device-only", "-c", os.path.join(CSRC, s), "-o", str(tmp / (s + ".o")),
                               "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in srcs]
    out = {}
    for s, p in zip(srcs, procs):
        _, err = p.communicate(timeout=3000)
        assert p.returncode == 0, err[-2000:]
        out[s] = parse(err)
    return out


def twins_and_plain(reports):
    for bd, plain in UNITS.items():
        base = {key(s)[:2]: r for s, r in reports[plain].items() if key(s) and not key(s)[2]}
        for s, r in sorted(reports[bd].items()):
            k = key(s)
            assert k and k[2], s
            yield s, r, base[k[:2]]


def test_every_form_has_its_twin_at_12_levels(reports):
    n = {}
    for s, _, _ in twins_and_plain(reports):
        kernel = key(s)[0]
        assert maxl(key(s)) == 12, s
        n[kernel] = n.get(kernel, 0) + 1
    assert n == COUNT
    # ... and they are the plain units' 12-level instantiations, one for one
    for bd, plain in UNITS.items():
        twelve = sorted(key(s)[:2] for s in reports[plain] if key(s) and maxl(key(s)) == 12)
        assert twelve == sorted(key(s)[:2] for s in reports[bd])


def test_no_twin_needs_more_scratch_or_spills_more_than_its_plain_kernel(reports):
    for s, twin, plain in twins_and_plain(reports):
        for fig in ("ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill"):
            assert twin[fig] <= plain[fig], (s, fig, twin, plain)
        assert twin["AGPRs"] == plain["AGPRs"] == 0, (s, twin, plain)
        assert twin["Occupancy [waves/SIMD]"] >= plain["Occupancy [waves/SIMD]"], (s, twin, plain)
        assert twin["LDS Size [bytes/block]"] == plain["LDS Size [bytes/block]"] + MEMBER_WORDS, (s, twin, plain)


def test_fresh_compile_reports_the_committed_figures(reports):
    c = committed()
    fresh = {s: r for bd in UNITS for s, r in reports[bd].items()}
    assert sorted(c) == sorted(fresh) and len(c) == sum(COUNT.values())
    for k in c:
        assert fresh[k] == c[k], (k, fresh[k], c[k])
        assert {"VGPRs", "TotalSGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"} <= set(c[k]), k
