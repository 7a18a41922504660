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


# ---- what tests/test_gpu_batched_edges.py runs on the GPU, as the planner answers it
E77 = Qu(7, 7)
LIMBS = {E43: 1, E77: 2, E88: 3}


def tags(ea, eb, grow=13):
    """the exact product and an accumulator of `grow` - 1 more bits: the linear class for K < 2^(grow - 1)"""
    return dict(mul_args=Tags(ea.intBits + eb.intBits + 1, ea.fracBits + eb.fracBits), add_args=[Qu(ea.intBits + eb.intBits + grow, ea.fracBits + eb.fracBits)])


def roomy(ea, eb, grow=13):
    """a C that holds every dot product of tags(ea, eb, grow), at the coarser operand's resolution"""
    return Qu(ea.intBits + eb.intBits + grow - 1, max(ea.fracBits, eb.fracBits))


# name -> (A element, B element, the largest K with min(LA, LB) * K <= 2^17 - 1)
BOUND = {"1x1": (E43, E43, 131071), "2x2": (E77, E77, 65535), "3x3": (E88, E88, 43690), "3x1": (E88, E43, 131071)}


def bound_case(name, over=0):
    """descriptor and C of a member of (3, 2, Kmax + over).  The accumulator and C hold Kmax * a * b exactly.  The single-limb
    pair's 32-bit epilogue takes a C of at most 30 value bits: Qu<26,0>, six fraction bits below the product's — a floor that is
    exact where one factor is the format's minimum, -2^7."""
    ea, eb, K = BOUND[name]
    kw = tags(ea, eb, 18)
    ec = Qu(26, 0) if name == "1x1" else kw["add_args"][0]
    return ea, eb, ec, K, lower(ea, eb, ec, 3, 2, K + over, **kw)


def test_the_one_launch_form_ends_at_the_exactness_bound():
    batch = 2
    for name in BOUND:
        ea, eb, _, K, d = bound_case(name)
        assert min(LIMBS[ea], LIMBS[eb]) * K <= 2 ** 17 - 1 < min(LIMBS[ea], LIMBS[eb]) * (K + 1)
        st, info = capi.classify_batched_status(d, batch)
        assert st == capi.QG_OK and list(info.limbs) == [LIMBS[ea], LIMBS[eb]] and capi.classify_batched_launches(d, batch) == 1, (name, info.reason)
        assert b"one block-diagonal launch" in bytes(info.reason)
        over = bound_case(name, 1)[4]
        st, info = capi.classify_batched_status(over, batch)
        assert st == capi.QG_OK and capi.classify_batched_launches(over, batch) > batch and b"k-chunk" in bytes(info.reason), (name, info.reason)


def test_all_nine_limb_pairs_take_one_launch():
    seen = set()
    for ea in (E43, E77, E88):
        for eb in (E43, E77, E88):
            for ta in (False, True):
                d = lower(ea, eb, roomy(ea, eb), 65, 33, 193, transposed_a=ta, **tags(ea, eb))
                for batch in (2, 9):
                    st, info = capi.classify_batched_status(d, batch)
                    assert st == capi.QG_OK and list(info.limbs) == [LIMBS[ea], LIMBS[eb]], info.reason
                    assert capi.classify_batched_launches(d, batch) == 1 and b"64x64" in bytes(info.reason), info.reason
                seen.add(tuple(info.limbs))
    assert len(seen) == 9


def test_a_member_of_eighteen_tile_rows_stays_in_one_launch():
    M, N, K, batch = 1089, 65, 65, 2
    d = lower(E43, E43, roomy(E43, E43), M, N, K, **tags(E43, E43))
    st, info = capi.classify_batched_status(d, batch)
    assert st == capi.QG_OK and capi.classify_batched_launches(d, batch) == 1 and b"64x64" in bytes(info.reason)
    # single limb: 18 x 2 tiles of 64x64 per member on one 128-byte k-tile; C in a 4-byte container (Qu<20,3>: 24 bits)
    assert list(info.packed_bytes) == [batch * 18 * 64 * 128, batch * 2 * 64 * 128, batch * 18 * 2 * 64 * 64 * 4]
    d = lower(E88, E88, roomy(E88, E88), M, N, K, **tags(E88, E88))
    st, info = capi.classify_batched_status(d, batch)
    assert st == capi.QG_OK and capi.classify_batched_launches(d, batch) == 1 and b"64x64" in bytes(info.reason)
    # three limbs: two 64-byte k-tiles, three planes per member and ONE trailer; C in an 8-byte container (Qu<28,8>: 37 bits)
    assert list(info.packed_bytes) == [batch * 3 * 18 * 64 * 128 + 256, batch * 3 * 2 * 64 * 128 + 256, batch * 18 * 2 * 64 * 64 * 8]


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
