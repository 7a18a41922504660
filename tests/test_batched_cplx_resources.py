"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of the combine pass of the stacked batched plans
(k_stack_combine_bd, qublas_amd/csrc/qg_combine_bd.hip: QG_OPT_BATCHED_STACKED): both instantiations — complex members, and the one
that serves both mixed orders — use no scratch and spill no register, keep the one 64 x 65 int64 transpose tile in LDS, and every
figure of a fresh compile — registers, occupancy, LDS — equals the committed report profiles/batched_cplx_kernel_resources.txt.
hipcc cross-compiles for gfx950 without a GPU: CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNELS = ["_ZN12_GLOBAL__N_118k_stack_combine_bdILb1EEEv13QStackCombine", "_ZN12_GLOBAL__N_118k_stack_combine_bdILb0EEEv13QStackCombine"]
LDS = 64 * 65 * 8


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
    return parse(open(os.path.join(ROOT, "profiles", "batched_cplx_kernel_resources.txt")).read())


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    tmp = tmp_path_factory.mktemp("batched_cplx")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "--cuda-device-only", "-c", os.path.join(CSRC, "qg_combine_bd.hip"),
                        "-o", str(tmp / "qg_combine_bd.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0, p.stderr[-2000:]
    return parse(p.stderr)


def check(kernels):
    assert sorted(kernels) == sorted(KERNELS), sorted(set(kernels) ^ set(KERNELS))
    for k in KERNELS:
        r = kernels[k]
        assert r["ScratchSize [bytes/lane]"] == 0, (k, r)
        assert r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        assert r["LDS Size [bytes/block]"] == LDS, (k, r)
        assert r["Occupancy [waves/SIMD]"] >= 4, (k, r)   # (four workgroups of four waves per CU is what the LDS tile allows)


def test_no_scratch_no_spills_in_every_instantiation(report):
    check(report)


def test_fresh_compile_reports_the_committed_figures(report):
    c = committed()
    assert sorted(c) == sorted(report)
    for k in c:
        assert report[k] == c[k], (k, report[k], c[k])
        assert {"VGPRs", "AGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]"} <= set(c[k]), k


def test_committed_report_is_clean_itself():
    c = committed()
    assert len(c) == 2
    check(c)
