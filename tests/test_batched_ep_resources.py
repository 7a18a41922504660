"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of the kernels that run element-wise chains on batched plans:
the 10 instantiations of k_mfma_ep_bd (qg_mfma_ep_bd.hip: the chain fused into the block-diagonal launch) and the block-diagonal
passes k_eltwise_bd and k_approx_bd<int32_t / int64_t> (qg_eltwise.hip, qg_approx.hip).  No scratch and no spilled register anywhere; the fused
kernels' static LDS no larger than that of the k_mfma_bd kernel of the same geometry (profiles/batched_kernel_resources.txt, which
tests/test_batched_resources.py holds against a fresh compile); and every figure of a fresh compile — registers, occupancy, LDS —
equal to the committed report profiles/batched_ep_kernel_resources.txt.  hipcc cross-compiles for gfx950 without a GPU: CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
SOURCES = ["qg_mfma_ep_bd.hip", "qg_eltwise.hip", "qg_approx.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the two pass files hold the plain and the other member forms' kernels too: this module is about these
KNOWN = re.compile(r"\dk_(mfma_ep_(bd|grp)I|eltwise(_bd|_grp)?E|approx(_bd|_grp)?I|pack_eE)")
MINE = re.compile(r"k_(mfma_ep|eltwise|approx)_bd[EI]")
# (LA, LB, BK, TI, TJ, SA, SB): the ten geometries of the block-diagonal launch (tests/test_batched_resources.py)
GEOMETRIES = ([(1, 1, 128, 1, 1, 1, 1)] +
              [(la, lb, 64, 1, 1, la, lb) for la in (1, 2, 3) for lb in (1, 2, 3) if la * lb > 1] + [(2, 2, 64, 1, 1, 3, 3)])
PASSES = ["_ZN12_GLOBAL__N_112k_eltwise_bdE14QEltwiseBdArgs", "_ZN12_GLOBAL__N_111k_approx_bdIiEEv13QApproxBdArgs", "_ZN12_GLOBAL__N_111k_approx_bdIlEEv13QApproxBdArgs"]


def fused(la, lb, bk, ti, tj, sa, sb):
    return f"_ZN12_GLOBAL__N_112k_mfma_ep_bdILi{la}ELi{lb}ELi{bk}ELi2ELi2ELi{ti}ELi{tj}ELi3ELi{sa}ELi{sb}EEEv13QMfmaEpBdArgs"


def plain_bd(la, lb, bk, ti, tj, sa, sb):
    return f"_ZN12_GLOBAL__N_19k_mfma_bdILi{la}ELi{lb}ELi{bk}ELi2ELi2ELi{ti}ELi{tj}ELi3ELi{sa}ELi{sb}EEEv9QMfmaArgs"


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


def committed(name):
    return parse(open(os.path.join(ROOT, "profiles", name)).read())


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    out = {}
    tmp = tmp_path_factory.mktemp("batched_ep")
    procs = [subprocess.Popen([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-device-only", "-c", os.path.join(CSRC, s),
                               "-o", str(tmp / (s + ".o")), "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for s in SOURCES]
    for s, p in zip(SOURCES, procs):
        _, err = p.communicate(timeout=1800)
        assert p.returncode == 0, err[-2000:]
        every = parse(err)
        assert all(KNOWN.search(k) for k in every), sorted(every)   # nothing but the chain kernels lives in these files
        out.update({k: v for k, v in every.items() if MINE.search(k)})
    return out


def check(kernels):
    bd = committed("batched_kernel_resources.txt")
    names = [fused(*g) for g in GEOMETRIES] + PASSES
    assert sorted(kernels) == sorted(names), sorted(set(kernels) ^ set(names))
    for k in names:
        r = kernels[k]
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
    for g in GEOMETRIES:
        assert kernels[fused(*g)]["LDS Size [bytes/block]"] <= bd[plain_bd(*g)]["LDS Size [bytes/block]"], g


def test_no_scratch_no_spills_and_lds_of_the_plain_block_diagonal_kernel(report):
    check(report)


def test_fresh_compile_reports_the_committed_figures(report):
    c = committed("batched_ep_kernel_resources.txt")
    assert sorted(c) == sorted(report)
    for k in c:
        assert report[k] == c[k], (k, report[k], c[k])
        assert {"VGPRs", "AGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]"} <= set(c[k]), k


def test_committed_report_is_clean_itself():
    c = committed("batched_ep_kernel_resources.txt")
    assert len(c) == 13
    check(c)
