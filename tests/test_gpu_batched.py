"""Batched Qgemul on the GPU (run with -m gpu): `batch` GEMMs of one descriptor at constant strides.  Every case is compared, member by
member, with the oracle (qoracle_gemm) AND byte for byte with qgemul_execute + qgemul_unpack_c of that member through a plain
plan.  The shapes are the smallest at which the block-diagonal walk (1 x 1, 2 x 1 and 3 x 3 tiles per member; batches that are no
multiple of the 8 XCD residue classes; more workgroups than CUs), the padding (ragged M, N, K) or the stack-wide data (ONE plane
mask and ONE row-sum array for all members) can go wrong.  Host buffers carry poison between the members; C's gaps must survive."""
import json
import os
import subprocess

import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, lower

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

E43, E88, E77, U8, Q78 = Qu(4, 3), Qu(8, 8), Qu(7, 7), Qu(8, 0, False), Qu(7, 8)
# name -> (A element, B element, C element, lowering keywords, transposed A, limbs the planner must report)
FORMATS = {
    "e43_c1byte": (E43, E43, Qu(4, 3), dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)]), False, [1, 1]),
    "e88_3x3": (E88, E88, Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), False, [3, 3]),
    "e77_2x2": (E77, E77, Qu(20, 7), dict(mul_args=Tags(15, 14), add_args=[Qu(27, 14)]), False, [2, 2]),
    "u8_centred": (U8, U8, Qu(26, 0, False), dict(mul_args=Tags(16, 0, False), add_args=[Qu(28, 0, False)]), False, [1, 1]),
    "q78_centred": (Q78, Q78, Qu(20, 8), dict(mul_args=Tags(15, 16), add_args=[Qu(28, 16)]), False, [2, 2]),
    "e88_x_e43_3x1": (E88, E43, Qu(20, 8), dict(mul_args=Tags(13, 11), add_args=[Qu(25, 11)]), False, [3, 1]),
    "e88_3x3_tn": (E88, E88, Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), True, [3, 3]),
}
SHAPES = [(1, 1, 1), (3, 5, 7), (64, 64, 64), (65, 33, 100), (129, 130, 65)]
BATCHES = (1, 2, 7, 9)
POISON = 0x5a


def extents(d, lda=0, ldb=0, ldc=0):
    ra, ca = (d.K, d.M) if d.transA else (d.M, d.K)
    return (ca - 1) * (lda or ra) + ra, (d.N - 1) * (ldb or d.K) + d.K, (d.N - 1) * (ldc or d.M) + d.M


def host_batch(oracle, e, batch, ext, stride, seed, dists):
    """a host buffer of `batch` members at `stride` elements: member b filled by the oracle's generator, poison between the members"""
    buf = np.empty((batch - 1) * stride + ext, dtype=oracle.host_dtype(e))
    buf.view(np.uint8)[:] = POISON
    members = []
    for b in range(batch):
        m = oracle.fill(e, ext, seed + 17 * b, dists[b % len(dists)])
        buf[b * stride:b * stride + ext] = m
        members.append(m)
    return buf, members


def run_batched_plan(ctx, oracle, d, ec, batch, A, B, strides, ld=(0, 0, 0)):
    """pack_batched + execute_batched + unpack_c_batched into a poisoned C; returns (C buffer, the plan's launch count)"""
    extC = extents(d, *ld)[2]
    C = np.empty((batch - 1) * strides[2] + extC, dtype=oracle.host_dtype(ec))
    C.view(np.uint8)[:] = POISON
    plan = capi.BatchedPlan(ctx, d, batch)
    pb = plan.info.packed_bytes
    bufs = [ctx.alloc(max(16, A.nbytes)), ctx.alloc(max(16, B.nbytes)), ctx.alloc(max(16, C.nbytes)), ctx.alloc(max(16, pb[0])), ctx.alloc(max(16, pb[1])), ctx.alloc(max(16, pb[2]))]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        ctx.h2d(dA, A.view(np.uint8)); ctx.h2d(dB, B.view(np.uint8)); ctx.h2d(dC, C.view(np.uint8))
        plan.pack(capi.OPERAND_A, dA, pA, strides[0], ld[0])
        plan.pack(capi.OPERAND_B, dB, pB, strides[1], ld[1])
        plan.execute(pC, pA, pB)
        plan.unpack_c(pC, dC, strides[2], ld[2])
        ctx.sync()
        ctx.d2h(C.view(np.uint8), dC)
        return C, plan.launches
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


def run_plain_members(ctx, oracle, d, ec, membersA, membersB, ld=(0, 0, 0)):
    """every member through a PLAIN plan: qgemul_pack, qgemul_execute, qgemul_unpack_c; tight C (ld[2] applies to the batched arm only)"""
    plan = capi.Plan(ctx, d)
    pb = plan.info.packed_bytes
    n = d.M * d.N
    out = []
    bufs = [ctx.alloc(max(16, membersA[0].nbytes)), ctx.alloc(max(16, membersB[0].nbytes)), ctx.alloc(max(16, n * plan.info.host_elem_bytes[2])),
            ctx.alloc(max(16, pb[0])), ctx.alloc(max(16, pb[1])), ctx.alloc(max(16, pb[2]))]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        for a, b in zip(membersA, membersB):
            ctx.h2d(dA, a.view(np.uint8)); ctx.h2d(dB, b.view(np.uint8))
            plan.pack(capi.OPERAND_A, dA, pA, ld[0])
            plan.pack(capi.OPERAND_B, dB, pB, ld[1])
            plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC, 0)
            ctx.sync()
            c = np.zeros(n, dtype=oracle.host_dtype(ec))
            ctx.d2h(c.view(np.uint8), dC)
            out.append(c)
        return out
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


def expected_buffer(oracle, d, ec, batch, membersC, stride, ldc=0):
    """what the batched C buffer must hold: the members at their stride (columns at ldc), poison everywhere else"""
    ext = (d.N - 1) * (ldc or d.M) + d.M
    exp = np.empty((batch - 1) * stride + ext, dtype=oracle.host_dtype(ec))
    exp.view(np.uint8)[:] = POISON
    for b in range(batch):
        for j in range(d.N):
            o = b * stride + j * (ldc or d.M)
            exp[o:o + d.M] = membersC[b][j * d.M:(j + 1) * d.M]
    return exp


@pytest.fixture(scope="module")
def ctx():
    with capi.Context() as c:
        yield c


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_one_launch_form_vs_oracle_and_plain_plan(ctx, oracle, fmt, shape):
    ea, eb, ec, kw, ta, limbs = FORMATS[fmt]
    M, N, K = shape
    d = lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)
    assert list(capi.classify_batched_status(d, 2)[1].limbs) == limbs
    extA, extB, extC = extents(d)
    strides = (extA, extB, extC)
    nb = max(BATCHES)
    A, mA = host_batch(oracle, ea, nb, extA, extA, 100, (0, 1))
    B, mB = host_batch(oracle, eb, nb, extB, extB, 200, (0, 1))
    exp = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]                 # computed once, shared by every batch count
    plain = run_plain_members(ctx, oracle, d, ec, mA, mB)
    for b in range(nb):
        assert plain[b].tobytes() == exp[b].tobytes(), (fmt, shape, b)
    for batch in BATCHES:
        got, launches = run_batched_plan(ctx, oracle, d, ec, batch, A[:(batch - 1) * extA + extA], B[:(batch - 1) * extB + extB], (extA, extB, extC))
        assert launches == 1, (fmt, shape, batch)
        assert got.tobytes() == expected_buffer(oracle, d, ec, batch, exp, extC).tobytes(), (fmt, shape, batch)


@pytest.mark.parametrize("fmt", ["e43_c1byte", "e88_3x3"])
def test_more_workgroups_than_cus(ctx, oracle, fmt):
    ea, eb, ec, kw, ta, _ = FORMATS[fmt]
    d = lower(ea, eb, ec, 64, 64, 64, **kw)
    batch, n = 300, 64 * 64
    A, mA = host_batch(oracle, ea, batch, n, n, 300, (0, 1))
    B, mB = host_batch(oracle, eb, batch, n, n, 400, (0, 1))
    got, launches = run_batched_plan(ctx, oracle, d, ec, batch, A, B, (n, n, n))
    assert launches == 1
    exp = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]
    assert got.tobytes() == np.concatenate(exp).tobytes()
    sample = [0, 1, 7, 8, 150, 299]
    plain = run_plain_members(ctx, oracle, d, ec, [mA[i] for i in sample], [mB[i] for i in sample])
    for i, c in zip(sample, plain):
        assert c.tobytes() == got[i * n:(i + 1) * n].tobytes(), i


def read_mask(ctx, plan, packed, operand):
    """the plane mask of a packed operand: the OR of the trailer's 64 words"""
    trailer = plan.packed_layout(operand)[0]
    assert trailer > 0
    w = np.zeros(64, dtype=np.uint32)
    ctx.d2h(w.view(np.uint8), packed + trailer)
    return int(np.bitwise_or.reduce(w))


@pytest.mark.parametrize("dists,third_plane", [((1, 0), True), ((1, 1), False)], ids=["small_then_full_range", "all_small"])
def test_plane_mask_is_the_or_over_every_member(ctx, oracle, dists, third_plane):
    """int<8,8> in three limb planes.  Member 0 small (|raw| < 2^8: the third plane is empty), member 1 full range: the stack's ONE mask
    must keep the third plane, which a per-member clear of the trailer (member 1 packed first, or member 0 last) would lose; with
    every member small the 2 x 2 partner of the launch pair does the work.  Either way every member equals the oracle."""
    ea, eb, ec, kw, _, _ = FORMATS["e88_3x3"]
    M, N, K, batch = 65, 33, 100, 2
    d = lower(ea, eb, ec, M, N, K, **kw)
    extA, extB, extC = extents(d)
    for order in (dists, dists[::-1]):                      # the full-range member last, then first
        A, mA = host_batch(oracle, ea, batch, extA, extA + 5, 500, order)
        B, mB = host_batch(oracle, eb, batch, extB, extB + 3, 600, order)
        plan = capi.BatchedPlan(ctx, d, batch)
        pb = plan.info.packed_bytes
        bufs = [ctx.alloc(A.nbytes), ctx.alloc(B.nbytes), ctx.alloc(batch * extC * np.dtype(oracle.host_dtype(ec)).itemsize), ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])]
        dA, dB, dC, pA, pB, pC = bufs
        try:
            ctx.h2d(dA, A.view(np.uint8)); ctx.h2d(dB, B.view(np.uint8))
            plan.pack(capi.OPERAND_A, dA, pA, extA + 5)
            plan.pack(capi.OPERAND_B, dB, pB, extB + 3)
            plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC, extC)
            ctx.sync()
            for operand, packed in ((capi.OPERAND_A, pA), (capi.OPERAND_B, pB)):
                mask = read_mask(ctx, plan, packed, operand)
                assert bool(mask & 4) == third_plane and (mask & 3) == 3, (order, operand, mask)
            got = np.zeros(batch * extC, dtype=oracle.host_dtype(ec))
            ctx.d2h(got.view(np.uint8), dC)
        finally:
            for p in bufs:
                ctx.free(p)
            plan.close()
        exp = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]
        assert got.tobytes() == np.concatenate(exp).tobytes(), order
        assert len(set(np.concatenate(exp).tolist())) > 100


@pytest.mark.parametrize("fmt", ["e43_c1byte", "q78_centred", "e88_3x3_tn"])
def test_strides_and_leading_dimensions_with_poison_between_the_members(ctx, oracle, fmt):
    ea, eb, ec, kw, ta, _ = FORMATS[fmt]
    M, N, K, batch = 65, 33, 100, 3
    d = lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)
    ld = ((K if ta else M) + 3, K + 5, M + 7)
    extA, extB, extC = extents(d, *ld)
    strides = (extA + 11, extB + 1, extC + 13)
    A, mA = host_batch(oracle, ea, batch, extA, strides[0], 700, (0,))       # (the padding rows inside a member hold generator values)
    B, mB = host_batch(oracle, eb, batch, extB, strides[1], 800, (0,))
    got, launches = run_batched_plan(ctx, oracle, d, ec, batch, A, B, strides, ld)
    assert launches == 1
    exp = []
    for a, b in zip(mA, mB):
        out = np.zeros(extC, dtype=oracle.host_dtype(ec))
        oracle.gemm(d, a, b, ec, lda=ld[0], ldb=ld[1], ldc=ld[2], out=out, nthreads=8)
        exp.append(np.concatenate([out[j * ld[2]:j * ld[2] + M] for j in range(N)]))
    assert got.tobytes() == expected_buffer(oracle, d, ec, batch, exp, strides[2], ld[2]).tobytes()
    plain = run_plain_members(ctx, oracle, d, ec, mA, mB, ld)
    for b in range(batch):
        assert plain[b].tobytes() == exp[b].tobytes()


C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
I16 = Qu(15, 0, True, TRN.TCPL, WRP.TCPL)
FALLBACKS = {
    # name -> (operand element, C element, lowering keywords, class, a word of the reason, launches per member)
    "tree_default_tags": (E88, E88, {}, 2, b"tree", 1),
    "complex_tf": (C5, C5, dict(mul_args=TFComplexMul()), 2, b"", 1),
    "ring_int16": (I16, I16, {}, 1, b"wrapping ring", 1),
    # linear class, single limb, but an exact LEFT shift into C that leaves the 32-bit epilogue: raw int32 dot products and a 64-bit
    # conversion pass per member, on the plain plan's own 128x128-tile layout (no block-diagonal form)
    "raw_pass_left_shift": (Qu(10, -3), Qu(24, 9), dict(mul_args=Tags(21, -6), add_args=[Qu(28, -6)]), 1, b"", 2),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallback_classes_run_member_by_member_through_the_same_entry(ctx, oracle, name):
    e, ec, kw, cls, why, per_member = FALLBACKS[name]
    M, N, K, batch = 33, 17, 40, 3
    d = lower(e, e, ec, M, N, K, **kw)
    st, info = capi.classify_batched_status(d, batch)
    assert st == capi.QG_OK and info.cls == cls and why in bytes(info.reason), info.reason
    extA, extB, extC = extents(d)
    strides = (extA + 2, extB + 3, extC + 4)
    A, mA = host_batch(oracle, e, batch, extA, strides[0], 900, (1,))
    B, mB = host_batch(oracle, e, batch, extB, strides[1], 950, (1,))
    got, launches = run_batched_plan(ctx, oracle, d, ec, batch, A, B, strides)
    assert launches == per_member * batch == capi.classify_batched_launches(d, batch)
    exp = [oracle.gemm(d, a, b, ec, nthreads=4) for a, b in zip(mA, mB)]
    assert got.tobytes() == expected_buffer(oracle, d, ec, batch, exp, strides[2]).tobytes()
    plain = run_plain_members(ctx, oracle, d, ec, mA, mB)
    for b in range(batch):
        assert plain[b].tobytes() == exp[b].tobytes()


def test_plain_and_batched_entry_points_refuse_each_other(ctx):
    import ctypes as C
    d = lower(E43, E43, Qu(4, 3), 64, 64, 64, mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
    bp, pp = capi.BatchedPlan(ctx, d, 2), capi.Plan(ctx, d)
    buf = ctx.alloc(1 << 16)
    L, v = capi.lib(), C.c_void_p
    try:
        assert L.qgemul_execute(bp.h, v(buf), v(buf), v(buf)) == capi.QG_EINVAL
        assert L.qgemul_pack(bp.h, 0, v(buf), 0, v(buf)) == capi.QG_EINVAL
        assert L.qgemul_unpack_c(bp.h, v(buf), v(buf), 0) == capi.QG_EINVAL
        assert L.qgemul_fill_packed(bp.h, 0, 1, 0, v(buf)) == capi.QG_EINVAL
        ms = C.c_float()
        assert L.qgemul_time_execute(bp.h, v(buf), v(buf), v(buf), 0, 1, C.byref(ms)) == capi.QG_EINVAL
        assert L.qgemul_execute_batched(pp.h, v(buf), v(buf), v(buf)) == capi.QG_EINVAL
        assert L.qgemul_pack_batched(pp.h, 0, v(buf), 0, 4096, v(buf)) == capi.QG_EINVAL
        assert L.qgemul_unpack_c_batched(pp.h, v(buf), v(buf), 0, 4096) == capi.QG_EINVAL
        assert L.qgemul_time_execute_batched(pp.h, v(buf), v(buf), v(buf), 0, 1, C.byref(ms)) == capi.QG_EINVAL
        assert L.qgemul_plan_batched_launches(pp.h) == capi.QG_EINVAL
        # strides below the member's extent, 0 included
        assert L.qgemul_pack_batched(bp.h, 0, v(buf), 0, 4095, v(buf)) == capi.QG_EINVAL
        assert L.qgemul_pack_batched(bp.h, 1, v(buf), 0, 0, v(buf)) == capi.QG_EINVAL
        assert L.qgemul_unpack_c_batched(bp.h, v(buf), v(buf), 0, 4095) == capi.QG_EINVAL
        assert bp.time_execute(buf, buf + 16384, buf + 32768, 1, 2) > 0
    finally:
        ctx.free(buf)
        bp.close()
        pp.close()


def test_one_shot_replans_when_the_batch_count_changes(oracle):
    ea, eb, ec, kw, _, _ = FORMATS["q78_centred"]
    M, N, K = 65, 33, 100
    d = lower(ea, eb, ec, M, N, K, **kw)
    extA, extB, extC = extents(d)
    strides = (extC + 9, extA + 1, extB + 2)                                  # (C, A, B: the order of qgemul_run_batched)
    A, mA = host_batch(oracle, ea, 7, extA, strides[1], 40, (0, 1))
    B, mB = host_batch(oracle, eb, 7, extB, strides[2], 50, (0, 1))
    exp = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]
    try:
        for batch in (7, 2, 2, 7):
            out = np.empty((batch - 1) * strides[0] + extC, dtype=oracle.host_dtype(ec))
            out.view(np.uint8)[:] = POISON
            capi.run_batched(d, batch, out, A, B, *strides)
            assert out.tobytes() == expected_buffer(oracle, d, ec, batch, exp, strides[0]).tobytes(), batch
            # a plain qgemul_run of the same descriptor in between: the thread's cache holds one plan, batched or not
            one = capi.run(d, np.zeros(extC, dtype=oracle.host_dtype(ec)), mA[0], mB[0])
            assert one.tobytes() == exp[0].tobytes()
    finally:
        capi.run_release()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_batched_program(tmp_path, oracle):
    """tests/binding/amd_header_batched_run.cpp: QgemulBatched<tags...>(C, A, B) on 3-d tensors through include/QuBLAS_amd.h"""
    exe = tmp_path / "amd_header_batched_run"
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++23", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "binding", "amd_header_batched_run.cpp"), "-o", str(exe), "-L" + lib, "-lqugemm", "-Wl,-rpath," + lib])
    recs = {r["name"]: r for r in (json.loads(l) for l in subprocess.check_output([str(exe)], text=True).strip().splitlines())}
    assert sorted(recs) == ["e88_L_tn", "e88_default"], recs
    cases = {"e88_L_tn": (Qu(24, 8), dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), True, (2654435761, 0, 131072, 65536), (40503, 7, 131072, 65536)),
             "e88_default": (E88, {}, False, (37, 0, 8192, 4096), (53, 1, 8192, 4096))}
    for name, (ec, kw, ta, ga, gb) in cases.items():
        r = recs[name]
        M, N, K, batch = r["M"], r["N"], r["K"], r["batch"]
        d = lower(E88, E88, ec, M, N, K, transposed_a=ta, **kw)
        gen = lambda n, g: (((np.arange(n, dtype=np.uint64) * np.uint64(g[0]) + np.uint64(g[1])) % np.uint64(g[2])).astype(np.int64) - g[3]).astype(np.int32)
        A, B = gen(batch * M * K, ga), gen(batch * K * N, gb)
        exp = np.concatenate([oracle.gemm(d, A[b * M * K:(b + 1) * M * K], B[b * K * N:(b + 1) * K * N], ec) for b in range(batch)])
        assert r["C"] == exp.astype(np.int64).tolist(), name
        assert len(set(r["C"])) > 20
