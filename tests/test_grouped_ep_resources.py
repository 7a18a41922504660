"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of the kernels that run element-wise chains on grouped plans:
the 10 instantiations of k_mfma_ep_grp (qg_mfma_ep_grp.hip: the chain fused into the grouped launch) and the passes k_eltwise_grp
and k_approx_grp<int32_t / int64_t> (qg_eltwise.hip, qg_approx.hip).  No scratch and no spilled register anywhere; every fused kernel's static
LDS no larger and its occupancy no lower than those of its k_mfma_ep_bd twin, the batched kernel of the same geometry
(profiles/batched_ep_kernel_resources.txt, which tests/test_batched_ep_resources.py holds against a fresh compile); and every figure
of a fresh compile — registers, occupancy, LDS — equal to the committed report profiles/grouped_ep_kernel_resources.txt.  hipcc
cross-compiles for gfx950 without a GPU: CPU only.

What the occupancy check caught while the kernel was written: with the chain applied at a 64-bit launch-wide element index per
lane, hipcc kept a 64-bit byte offset per run and container alive through the chain (18 registers), and 1 x 3, 3 x 1, 2 x 2 and
2 x 2 on three-plane storage reported 122 + 48 registers, 2 waves per SIMD, against 105 + 48 and 3 waves of the twin.  The kernel
now puts the wave-uniform tile base into the base pointers and keeps a 32-bit byte offset per lane: 105 + 48, 3 waves."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
SOURCES = ["qg_mfma_ep_grp.hip", "qg_eltwise.hip", "qg_approx.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# the two pass files hold the plain and the other member forms' kernels too: this module is about these
KNOWN = re.compile(r"\dk_(mfma_ep_(bd|grp)I|eltwise(_bd|_grp)?E|approx(_bd|_grp)?I|pack_eE)")
MINE = re.compile(r"k_(mfma_ep|eltwise|approx)_grp[EI]")
# (LA, LB, BK, TI, TJ, SA, SB): the ten geometries of the grouped launch (tests/test_grouped_resources.py)
GEOMETRIES = ([(1, 1, 128, 1, 1, 1, 1)] +
              [(la, lb, 64, 1, 1, la, lb) for la in (1, 2, 3) for lb in (1, 2, 3) if la * lb > 1] + [(2, 2, 64, 1, 1, 3, 3)])
PASSES = ["_ZN12_GLOBAL__N_113k_eltwise_grpE15QEltwiseGrpArgs", "_ZN12_GLOBAL__N_112k_approx_grpIiEEv14QApproxGrpArgs", "_ZN12_GLOBAL__N_112k_approx_grpIlEEv14QApproxGrpArgs"]


def fused(la, lb, bk, ti, tj, sa, sb):
    return f"_ZN12_GLOBAL__N_113k_mfma_ep_grpILi{la}ELi{lb}ELi{bk}ELi2ELi2ELi{ti}ELi{tj}ELi3ELi{sa}ELi{sb}EEEv14QMfmaEpGrpArgs"


def twin(la, lb, bk, ti, tj, sa, sb):
    return f"_ZN12_GLOBAL__N_112k_mfma_ep_bdILi{la}ELi{lb}ELi{bk}ELi2ELi2ELi{ti}ELi{tj}ELi3ELi{sa}ELi{sb}EEEv13QMfmaEpBdArgs"


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
    tmp = tmp_path_factory.mktemp("grouped_ep")
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
    bd = committed("batched_ep_kernel_resources.txt")
    names = [fused(*g) for g in GEOMETRIES] + PASSES
    assert sorted(kernels) == sorted(names), sorted(set(kernels) ^ set(names))
    for k in names:
        r = kernels[k]
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
    for g in GEOMETRIES:
        assert kernels[fused(*g)]["LDS Size [bytes/block]"] <= bd[twin(*g)]["LDS Size [bytes/block]"], g


def check_occupancy(kernels):
    bd = committed("batched_ep_kernel_resources.txt")
    print({g: (kernels[fused(*g)]["Occupancy [waves/SIMD]"], bd[twin(*g)]["Occupancy [waves/SIMD]"]) for g in GEOMETRIES})   # (the figures first)
    for g in GEOMETRIES:
        mine, other = kernels[fused(*g)], bd[twin(*g)]
        assert mine["Occupancy [waves/SIMD]"] >= other["Occupancy [waves/SIMD]"], (g, mine, other)


def test_no_scratch_no_spills_and_lds_of_the_batched_twin(report):
    check(report)


def test_occupancy_of_the_batched_twin(report):
    check_occupancy(report)


def test_fresh_compile_reports_the_committed_figures(report):
    c = committed("grouped_ep_kernel_resources.txt")
    assert sorted(c) == sorted(report)
    for k in c:
        assert report[k] == c[k], (k, report[k], c[k])
        assert {"VGPRs", "AGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]"} <= set(c[k]), k


def test_committed_report_is_clean_itself():
    c = committed("grouped_ep_kernel_resources.txt")
    assert len(c) == 13
    check(c)


def test_committed_report_meets_the_occupancy_of_the_batched_twin():
    check_occupancy(committed("grouped_ep_kernel_resources.txt"))
