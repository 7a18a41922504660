"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of the 10 instantiations of k_mfma_grp (qg_mfma_grp.hip: the
grouped Qgemul's launch): no scratch, no spilled registers, and static LDS and occupancy no worse than the block-diagonal twin
k_mfma_bd of the same geometry (qg_mfma.hip, compiled in the same fixture) — in the compiler's output of this tree and in the
committed one (profiles/grouped_kernel_resources.txt).  hipcc cross-compiles for gfx950 without a GPU: CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# (LA, LB, BK, TI, TJ, SA, SB) on 2 x 2 waves, 64x64 tiles and a 3-stage ring: single limb on 128-byte k-tiles, the limb
# kernels on 64-byte ones, and the 2 x 2 partner of a 3 x 3 launch on three-plane storage
GEOMETRIES = ([(1, 1, 128, 1, 1, 1, 1)] +
              [(la, lb, 64, 1, 1, la, lb) for la in (1, 2, 3) for lb in (1, 2, 3) if la * lb > 1] + [(2, 2, 64, 1, 1, 3, 3)])


def grouped(la, lb, bk, ti, tj, sa, sb):
    return f"_ZN12_GLOBAL__N_110k_mfma_grpILi{la}ELi{lb}ELi{bk}ELi2ELi2ELi{ti}ELi{tj}ELi3ELi{sa}ELi{sb}EEEv12QMfmaGrpArgs"


def twin(la, lb, bk, ti, tj, sa, sb):
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


def committed():
    return parse(open(os.path.join(ROOT, "profiles", "grouped_kernel_resources.txt")).read())


def compile_report(src, out_dir):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-device-only", "-c", os.path.join(CSRC, src), "-o",
                        os.path.join(out_dir, src + ".o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    d = str(tmp_path_factory.mktemp("grouped"))
    return parse(compile_report("qg_mfma_grp.hip", d) + compile_report("qg_mfma.hip", d))


def check(kernels):
    assert len(GEOMETRIES) == 10
    assert sum(1 for k in kernels if "k_mfma_grp" in k) == 10, sorted(k for k in kernels if "k_mfma_grp" in k)
    for g in GEOMETRIES:
        b, t = kernels[grouped(*g)], kernels[twin(*g)]
        assert b["ScratchSize [bytes/lane]"] == 0, (g, b)
        assert b["VGPRs Spill"] == 0 and b["SGPRs Spill"] == 0, (g, b)
        assert b["LDS Size [bytes/block]"] <= t["LDS Size [bytes/block]"], (g, b, t)
        assert b["Occupancy [waves/SIMD]"] >= t["Occupancy [waves/SIMD]"], (g, b, t)


def test_no_scratch_no_spills_lds_and_occupancy_of_the_block_diagonal_twin(report):
    check(report)


def test_committed_report_is_clean_itself():
    c = committed()
    assert len(c) == 20
    check(c)
