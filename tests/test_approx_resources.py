"""hipcc's own resource report (-Rpass-analysis=kernel-resource-usage) of the two instantiations of k_approx (qg_approx.hip: 32-bit and
64-bit arithmetic): no scratch, no spilled registers, the LDS of the four tables, and the occupancy DESIGN.md §7b states — at least
3 waves per SIMD for the 32-bit form, at least 2 for the 64-bit form (16 values per lane, twice the registers each).  hipcc
cross-compiles for gfx950 without a GPU: CPU only.  The same report is kept in profiles/approx_kernel_resources.txt."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qublas_amd", "csrc", "qg_approx.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = {32: "_ZN12_GLOBAL__N_18k_approxIiEEv11QApproxArgs", 64: "_ZN12_GLOBAL__N_18k_approxIlEEv11QApproxArgs"}


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


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    obj = str(tmp_path_factory.mktemp("approx") / "approx.o")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-x", "hip", "-c", SRC, "-o", obj,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    # (the file holds the member forms k_approx_bd and k_approx_grp too: tests/test_batched_ep_resources.py, test_grouped_ep_resources.py)
    every = parse(r.stderr)
    assert all(re.search(r"\dk_approx(_bd|_grp)?I[il]E", k) for k in every) and len(every) == 6, sorted(every)   # nothing else lives in the file
    return {k: v for k, v in every.items() if re.search(r"\dk_approxI", k)}


def check(kernels):
    assert sorted(kernels) == sorted(NAMES.values()), sorted(kernels)
    for bits, name in NAMES.items():
        v = kernels[name]
        assert v["ScratchSize [bytes/lane]"] == 0, (name, v)
        assert v["VGPRs Spill"] == 0 and v["SGPRs Spill"] == 0, (name, v)
        assert v["Occupancy [waves/SIMD]"] >= (3 if bits == 32 else 2), (name, v)
        assert v["LDS Size [bytes/block]"] == 4 * (16 + 8 * 16) * 8, (name, v)   # four tables: thresholds + coefficients, 64-bit words


def test_no_scratch_no_spills_and_the_stated_occupancy(report):
    check(report)


def test_committed_report_says_the_same():
    check(parse(open(os.path.join(ROOT, "profiles", "approx_kernel_resources.txt")).read()))
