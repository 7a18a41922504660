"""The epilogue of k_mfma_k6 (qg_mfma_k6.hip) in the ISA hipcc emits for gfx950: the six accumulators recombine in 32-bit pieces.
Per output the three Karatsuba differences are 32-bit subtractions and x = S00 + 2^6 c1 + 2^12 c2 + 2^18 c3 + 2^24 S22 is four
v_mad_u64_u32 (24 outputs per wave and tile: at least 96 in every instantiation); the only 64-bit subtraction left per output is
the one that takes the row term from the column term (the 64-bit form needed four: v_subb_co_u32 counts the high halves), and the
accumulators are no longer sign-extended one by one (v_ashrrev_i32 by 31: 144 of them before).  hipcc cross-compiles without a GPU:
CPU only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "qublas_amd", "csrc", "qg_mfma_k6.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
OUTPUTS = 24      # per lane and tile: 3 x 2 tiles of 16 x 16, 4 rows each


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("needs hipcc")
    asm = str(tmp_path_factory.mktemp("k6epi") / "k6.s")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-x", "hip", "--cuda-device-only", "-S", SRC, "-o", asm],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur = {}, None
    for ln in open(asm):
        m = re.match(r"^(_Z\w*k_mfma_k6\w*):", ln)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif ln.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            ins = ln.split(";")[0].strip()
            if ins and not ins.startswith("."):
                cur.append(ins)
    return out


def test_recombination_in_32_bit_pieces(kernels):
    assert len(kernels) == 4, sorted(kernels)
    for name, ins in kernels.items():
        n = lambda op: sum(1 for s in ins if s.split()[0] == op)
        assert n("v_mad_u64_u32") >= 4 * OUTPUTS, (name, n("v_mad_u64_u32"))
        if "ILb1E" in name:      # FAST: shift and clamp follow; the general routine of the others subtracts in 64 bits itself
            assert n("v_subb_co_u32_e32") + n("v_subb_co_u32_e64") <= 2 * OUTPUTS, (name, n("v_subb_co_u32_e32"))
        sign_ext = sum(1 for s in ins if s.startswith("v_ashrrev_i32") and re.search(r"\s31,", s))
        assert sign_ext <= OUTPUTS, (name, sign_ext)
