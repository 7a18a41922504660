"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of every instantiation of k_mfma_ring (qg_mfma_ring.hip): no
scratch, no spilled vector registers, at most 256 vector registers and two waves per SIMD (the 8 waves of a workgroup), and the LDS
ring — three stages where they fit, two for the 7 and 8 planes of a 32-bit ring — inside the 160 KiB of a CU.  hipcc cross-compiles
for gfx950 without a GPU: CPU only.  The same report is kept in profiles/ring_kernel_resources.txt."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qublas_amd", "csrc", "qg_mfma_ring.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    obj = str(tmp_path_factory.mktemp("ring") / "ring.o")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", SRC, "-o", obj,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
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


def instantiations():
    """(LA, LB, weights) the launcher dispatches to: planes of at most the ring's L <= 4 digits, weights min(L, LA + LB - 1)"""
    out = set()
    for L in (1, 2, 3, 4):
        for la in range(1, L + 1):
            for lb in range(1, L + 1):
                out.add((la, lb, min(L, la + lb - 1)))
    return sorted(out)


def test_every_instantiation_fits_two_waves_per_simd(report):
    ring = {n: v for n, v in report.items() if "k_mfma_ring" in n}
    want = instantiations()
    assert len(want) == 20 and len(ring) == len(want), sorted(ring)
    for la, lb, w in want:
        name = "_ZN12_GLOBAL__N_111k_mfma_ringILi%dELi%dELi%dEEEv9QRingArgs" % (la, lb, w)
        assert name in ring, name
    for name, v in ring.items():
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0, (name, v)
        assert v["VGPRs"] + v.get("AGPRs", 0) <= 256, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= 2, (name, v)


def test_lds_ring_fits_a_compute_unit():
    src = open(SRC).read()
    assert re.search(r"enum \{ QG_RING_VARIANT = 12, QG_RING_TM = 128, QG_RING_TN = 128, QG_RING_BK = 64 \};",
                     open(os.path.join(os.path.dirname(SRC), "qg_geom.h")).read())
    lds_max = eval(re.search(r"constexpr int LDS_MAX = ([0-9* ]+);", src).group(1))
    assert lds_max == 160 * 1024
    assert "return 3 * (LA * TM + LB * TN) * BK <= LDS_MAX ? 3 : 2;" in src          # ring_stages
    for la, lb, _ in instantiations():
        stage = (la + lb) * 128 * 64
        stages = 3 if 3 * stage <= lds_max else 2
        assert stages * stage <= lds_max, (la, lb)
        assert (stages - 1) * (la + lb) < 64                                          # outstanding LDS-DMA pieces: vmcnt has 6 bits
    assert 2 * 8 * 128 * 64 == 128 * 1024                                             # 4 + 4 planes: two stages of 64 KiB
