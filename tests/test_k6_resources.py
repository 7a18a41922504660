"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of every instantiation of k_mfma_k6 (qg_mfma_k6.hip): no
scratch, no spilled vector registers, at most 256 vector registers (two waves per SIMD: the two wave groups of a workgroup share
each SIMD), and the three-buffer LDS ring inside the 160 KiB of a CU.  hipcc cross-compiles for gfx950 without a GPU: CPU only.
The same report is kept in profiles/k6_kernel_resources.txt."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qublas_amd", "csrc", "qg_mfma_k6.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    obj = str(tmp_path_factory.mktemp("k6") / "k6.o")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", SRC, "-o", obj,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", ln)
        if m:
            cur = kernels.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}([A-Za-z /\[\]]+?): (\d+)", ln)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return kernels


def test_every_instantiation_fits_two_waves_per_simd(report):
    k6 = {n: v for n, v in report.items() if "k_mfma_k6" in n}
    assert len(k6) == 4, sorted(report)       # FAST x {4, 8}-byte C
    for name, v in k6.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0, (name, v)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 2, (name, v)


def test_lds_ring_fits_a_compute_unit():
    src = open(SRC).read()
    tm, tn, bk = (int(x) for x in re.search(r"constexpr int TM = (\d+), TN = (\d+), BK = (\d+);", src).groups())
    nbuf = int(re.search(r"constexpr int NBUF = (\d+);", src).group(1))
    assert (tm, tn, bk) == (96, 128, 64)
    assert nbuf * 3 * (tm + tn) * bk <= 160 * 1024     # dynamic LDS of the launch: NBUF buffers of 3 + 3 planes
