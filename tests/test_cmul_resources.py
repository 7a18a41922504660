"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of the two instantiations of k_eltwise_cplx (qg_eltwise_cplx.hip:
32-bit and 64-bit arithmetic): no scratch, no spilled registers, and at least the occupancy the committed report
(profiles/cmul_kernel_resources.txt, the same compiler output) shows.  hipcc cross-compiles for gfx950 without a GPU: CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qublas_amd", "csrc", "qg_eltwise_cplx.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = {32: "_ZN12_GLOBAL__N_114k_eltwise_cplxIiEEv13QCplxPassArgs", 64: "_ZN12_GLOBAL__N_114k_eltwise_cplxIlEEv13QCplxPassArgs"}


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
    return parse(open(os.path.join(ROOT, "profiles", "cmul_kernel_resources.txt")).read())


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    obj = str(tmp_path_factory.mktemp("cmul") / "cmul.o")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", SRC, "-o", obj,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return parse(r.stderr)


def check(kernels, floor):
    assert sorted(kernels) == sorted(NAMES.values()), sorted(kernels)
    for bits, name in NAMES.items():
        v = kernels[name]
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["LDS Size [bytes/block]"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= floor[name]["Occupancy [waves/SIMD]"], (name, v)


def test_no_scratch_no_spills_and_the_committed_occupancy(report):
    check(report, committed())


def test_committed_report_is_clean_itself():
    c = committed()
    check(c, c)
