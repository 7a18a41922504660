"""The batched Qgemul's planner on the CPU (qgemul_classify_batched, qgemul_classify_batched_launches, the argument checks of
qgemul_run_batched: pure host code): packed sizes of the whole batch, one launch for small linear-class members and a loop for
everything else, every QG_EINVAL of include/qgemul.h, batch = 1 against the plain plan, and the three lowerings of QgemulBatched
(qublas_amd/desc.py, include/QuBLAS_amd.h, include/qgemul_reference_binding.hpp) against the Qgemul lowering of one member."""
import json
import os
import subprocess

import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, lower

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
REF_INC = os.environ.get("REF_INC", "/root/reference/include")

E43, E88, W16 = Qu(4, 3), Qu(8, 8), Qu(16, 3)
L43 = dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
L88 = dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
I16 = Qu(15, 0, True, TRN.TCPL, WRP.TCPL)


def up(x, m):
    return (x + m - 1) // m * m


def test_packed_bytes_are_batch_times_the_tile_padded_member():
    for M, N, K in ((64, 64, 64), (1, 1, 1), (65, 33, 100), (129, 130, 65)):
        d = lower(E43, E43, W16, M, N, K, **L43)
        for batch in (1, 2, 7, 300):
            st, info = capi.classify_batched_status(d, batch)
            assert st == capi.QG_OK and capi.classify_batched_launches(d, batch) == 1, info.reason
            # single limb: 64x64 tiles on 128-byte k-tiles, one byte per element; C in a 4-byte container (Qu<16,3>: 20 bits)
            assert list(info.packed_bytes) == [batch * up(M, 64) * up(K, 128), batch * up(N, 64) * up(K, 128), batch * up(M, 64) * up(N, 64) * 4], (M, N, K, batch)
            assert info.ops == 2.0 * M * N * K * batch
    # three limbs: the planes of every member, then ONE 256-byte plane-mask trailer for the stack
    d = lower(E88, E88, Qu(24, 8), 65, 33, 100, **L88)
    st, info = capi.classify_batched_status(d, 7)
    assert st == capi.QG_OK and list(info.limbs) == [3, 3]
    assert list(info.packed_bytes) == [7 * 3 * 128 * 128 + 256, 7 * 3 * 64 * 128 + 256, 7 * 128 * 64 * 8]   # (Qu<24,8>: 33 storage bits, 8-byte containers)
    # members of 256 x 256: 64x64 tiles as well (sixteen per member)
    d = lower(E43, E43, W16, 256, 256, 64, **L43)
    st, info = capi.classify_batched_status(d, 256)
    assert st == capi.QG_OK and list(info.packed_bytes) == [256 * 256 * 128, 256 * 256 * 128, 256 * 256 * 256 * 4] and b"64x64" in bytes(info.reason)


def test_one_launch_for_small_linear_members_and_the_loop_for_everything_else():
    assert capi.classify_batched_launches(lower(E43, E43, W16, 64, 64, 64, **L43), 9) == 1
    assert capi.classify_batched_launches(lower(E88, E88, Qu(24, 8), 64, 64, 64, **L88), 9) == 1
    tree = lower(E88, E88, E88, 33, 17, 40)
    assert capi.classify_batched_status(tree, 3)[1].cls == 2 and capi.classify_batched_launches(tree, 3) == 3
    cplx = lower(C5, C5, C5, 33, 17, 40, mul_args=TFComplexMul())
    assert capi.classify_batched_launches(cplx, 3) == 3
    ring = lower(I16, I16, I16, 33, 17, 40)
    assert b"wrapping ring" in bytes(capi.classify_batched_status(ring, 3)[1].reason) and capi.classify_batched_launches(ring, 3) == 3
    # a complex member of the linear class: MFMA kernel + combine pass per member
    cw = Qcomplex(Qu(18, 6, True, RND.POS_INF, SAT.TCPL), Qu(18, 6, True, RND.POS_INF, SAT.TCPL))
    c55 = Qcomplex(Qu(5, 5), Qu(5, 5))
    dl = lower(c55, c55, cw, 33, 17, 40)
    if capi.KERNEL_NAMES[capi.classify(dl).kernel] == "mfma_cplx":
        assert capi.classify_batched_launches(dl, 3) == 6
    # composite plans (K beyond the int32 accumulators' exact range): k-chunks x (sub-GEMMs + combine) per member
    comp = lower(E43, E43, Qu(30, 3), 64, 64, 140000, mul_args=Tags(9, 6), add_args=[Qu(27, 6)])
    n = capi.classify_batched_launches(comp, 2)
    assert n > 2 and n % 2 == 0
    # a left shift into C that leaves the single-limb kernels' 32-bit epilogue: raw dot products + a conversion pass per member, on the
    # plain plan's own layout (the batched tile choice does not stick to a member that has no one-launch form)
    raw = lower(Qu(10, -3), Qu(10, -3), Qu(24, 9), 33, 17, 40, mul_args=Tags(21, -6), add_args=[Qu(28, -6)])
    assert capi.KERNEL_NAMES[capi.classify(raw).kernel] == "mfma_i8" and capi.classify_batched_launches(raw, 3) == 6
    assert list(capi.classify_batched_status(raw, 3)[1].packed_bytes) == [3 * ((b + 255) // 256 * 256) for b in capi.classify(raw).packed_bytes]
    # a member big enough for the two-group kernels runs on them, member by member
    big = lower(E43, E43, W16, 4096, 4096, 256, **L43)
    assert capi.classify_batched_launches(big, 2) == 2
    assert list(capi.classify_batched_status(big, 2)[1].packed_bytes) == [2 * b for b in capi.classify(big).packed_bytes]


def test_every_einval():
    d = lower(E43, E43, W16, 64, 64, 64, **L43)
    for batch in (0, -1):
        assert capi.classify_batched_status(d, batch)[0] == capi.QG_EINVAL
        assert capi.classify_batched_launches(d, batch) == capi.QG_EINVAL
    assert capi.classify_batched_status(d, 2 ** 31 - 1)[0] == capi.QG_OK          # one tile per member
    assert capi.classify_batched_status(d, 2 ** 31)[0] == capi.QG_EINVAL
    d4 = lower(E43, E43, W16, 65, 65, 64, **L43)                                   # four tiles per member
    assert capi.classify_batched_status(d4, 2 ** 29 - 1)[0] == capi.QG_OK
    assert capi.classify_batched_status(d4, 2 ** 29)[0] == capi.QG_EINVAL
    # strides (host elements): at least the member's extent, never 0 — refused before any device is touched
    M, N, K = 3, 5, 7
    ds = lower(E43, E43, W16, M, N, K, **L43)
    A, B, Cc = np.zeros(2 * M * K + 8, np.int32), np.zeros(2 * K * N + 8, np.int32), np.zeros(2 * M * N + 8, np.int32)
    ok = (M * N, M * K, K * N)
    for bad in ((0, ok[1], ok[2]), (ok[0], 0, ok[2]), (ok[0], ok[1], 0), (ok[0] - 1, ok[1], ok[2]), (ok[0], ok[1] - 1, ok[2]), (ok[0], ok[1], ok[2] - 1)):
        assert capi.run_batched_status(ds, 2, Cc, A, B, *bad) == capi.QG_EINVAL, bad
    # a leading dimension enlarges the extent: (cols - 1) * ld + rows
    assert capi.run_batched_status(ds, 2, Cc, A, B, (N - 1) * (M + 2) + M - 1, ok[1], ok[2], ldc=M + 2) == capi.QG_EINVAL
    assert capi.run_batched_status(ds, 2, Cc, A, B, ok[0], ok[1], ok[2], ldc=M - 1) == capi.QG_EINVAL
    assert capi.run_batched_status(ds, 0, Cc, A, B, *ok) == capi.QG_EINVAL
    assert capi.run_batched_status(ds, 2, Cc, A, B, *ok, flags=capi.OPT_ALL_DEVICES) == capi.QG_EUNSUPPORTED


def test_batch_of_one_classifies_like_the_plain_plan():
    cases = [lower(E43, E43, W16, 64, 64, 64, **L43), lower(E88, E88, Qu(24, 8), 65, 33, 100, **L88), lower(E88, E88, E88, 33, 17, 40),
             lower(C5, C5, C5, 33, 17, 40, mul_args=TFComplexMul()), lower(I16, I16, I16, 33, 17, 40), lower(E43, E43, W16, 4096, 4096, 256, **L43)]
    for d in cases:
        st, b = capi.classify_batched_status(d, 1)
        p = capi.classify(d)
        assert st == capi.QG_OK
        assert (b.cls, b.kernel, list(b.limbs), b.max_bits, list(b.host_elem_bytes)) == (p.cls, p.kernel, list(p.limbs), p.max_bits, list(p.host_elem_bytes))


# ---- the three lowerings: QgemulBatched's descriptor is byte for byte the one Qgemul lowers for one member
PROBED = {
    "e43_L_64x64x64_b7": (lower(E43, E43, W16, 64, 64, 64, **L43), 7, [64 * 64, 64 * 64, 64 * 64]),
    "e88_L_tn_33x17x40_b3": (lower(E88, E88, Qu(24, 8), 33, 17, 40, transposed_a=True, **L88), 3, [33 * 17, 40 * 33, 40 * 17]),
    "e88_default_3x5x7_b2": (lower(E88, E88, E88, 3, 5, 7), 2, [15, 21, 35]),
}


def _probe(tmp_path, src, extra=()):
    exe = tmp_path / os.path.splitext(src)[0]
    subprocess.check_call([CLANG, "-std=c++23", "-O0", "-w", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "tests", "binding"), *extra,
                           os.path.join(ROOT, "tests", "binding", src), "-o", str(exe)])
    return {l["name"]: l for l in (json.loads(x) for x in subprocess.check_output([str(exe)], text=True).strip().splitlines())}


def _check(recs):
    assert sorted(recs) == sorted(PROBED)
    for name, (d, batch, strides) in PROBED.items():
        r = recs[name]
        assert r["batched"] == r["member"], name
        assert r["batched"] == bytes(d).hex(), name
        assert (r["batch"], r["strides"]) == (batch, strides), name


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_lowers_the_member_descriptor(tmp_path):
    _check(_probe(tmp_path, "amd_header_batched_probe.cpp"))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_reference_binding_lowers_the_member_descriptor(tmp_path):
    if not os.path.exists(os.path.join(REF_INC, "QuBLAS.h")):
        pytest.skip("the reference header is not on this machine")
    _check(_probe(tmp_path, "ref_binding_batched_probe.cpp", ["-I" + REF_INC]))
