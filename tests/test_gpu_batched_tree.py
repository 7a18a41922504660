"""The one-launch TREE form of batched Qgemul on the GPU (QG_OPT_BATCHED_TREE; run with -m gpu): a batch whose member runs on a tiled
32-bit tree kernel as ONE launch of that kernel's batched twin (qublas_amd/csrc/qg_tree_bd.h).  Every comparison is byte for byte:
the flagged batched plan == the oracle (qoracle_gemm per member) == the unflagged batched plan ON THE SAME PACKED BUFFERS == a plain
plan per member.  The shapes are the smallest at which the walk over the members (one tile, 2 x 2 partial tiles, more than one group
of 16 tile rows, batches that are no multiple of the 8 XCD residue classes, more workgroups than CUs), the 12-level limit or the
members' strides can go wrong.  Host buffers and the packed C carry poison between the members; it must survive."""
import json
import os
import subprocess

import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, TFComplexMul, lower
from test_gpu_batched import CLANG, POISON, ROOT, expected_buffer, extents, host_batch, run_plain_members
from test_gpu_tree_levels import C5, CPLX, E88, E88Z, Q1516, REAL

pytestmark = pytest.mark.gpu
F = capi.OPT_BATCHED_TREE
E43 = Qu(4, 3)
PACKED_POISON = 0xA5
# name -> (element, lowering keywords, kernel, the end of the member's reason)
MEMBERS = {
    "e88_lj": (E88, {}, "tree_i32", "one format, SAT::TCPL, left-justified"),
    "e43_pk16": (E43, {}, "tree_i32", "one format, SAT::TCPL, left-justified, packed 16-bit"),
    "e88z_one_zero": (E88Z, {}, "tree_i32", "one format, SAT::ZERO"),
    "c5_tf": (C5, dict(mul_args=TFComplexMul()), "tree_cplx_i32", "fixed modes, one clamp, packed 16-bit"),
}
SHAPES = [(1, 1, 1), (64, 32, 32), (65, 33, 33), (3, 5, 7), (129, 130, 65), (17, 9, 4096)]
BATCHES = (1, 2, 7, 9)


@pytest.fixture(scope="module")
def ctx():
    with capi.Context() as c:
        yield c


def reason(info):
    return bytes(info.reason).rstrip(b"\0").decode()


def planned(d, batch, flags, form, kernel):
    """what the planner answers under the flag, asserted before any device work"""
    st, info = capi.classify_batched_status(d, batch, flags | F)
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == kernel, (st, info.reason)
    assert reason(info).startswith("batch in one launch; ") and reason(info).endswith(form), (info.reason, form)
    assert capi.classify_batched_launches(d, batch, flags | F) == 1 and capi.classify_batched_launches(d, batch, flags) == batch


def run_both(ctx, oracle, d, ec, batch, A, B, strides, ld=(0, 0, 0), flags=0, one_launch=True, packed_c=None, timed=False):
    """pack_batched once (through the flagged plan), then execute_batched + unpack_c_batched through the FLAGGED and through the UNFLAGGED
    batched plan on those same packed operands, each into its own poisoned packed C and poisoned host C.  Returns the two host C buffers
    (flagged, unflagged) and the two launch counts.  packed_c: a list that receives the flagged plan's packed C after the execute;
    timed: the flagged plan runs through qgemul_time_execute_batched instead"""
    extC = extents(d, *ld)[2]
    C = np.empty((batch - 1) * strides[2] + extC, dtype=oracle.host_dtype(ec))
    C.view(np.uint8)[:] = POISON
    on, off = capi.BatchedPlan(ctx, d, batch, flags | F), capi.BatchedPlan(ctx, d, batch, flags)
    pb = list(on.info.packed_bytes)
    bufs = [ctx.alloc(max(16, A.nbytes)), ctx.alloc(max(16, B.nbytes)), ctx.alloc(max(16, C.nbytes)), ctx.alloc(max(16, pb[0])), ctx.alloc(max(16, pb[1])), ctx.alloc(max(16, pb[2]))]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        assert pb == list(off.info.packed_bytes) and on.info.kernel == off.info.kernel
        assert on.launches == (1 if one_launch else off.launches)
        raw = np.full(max(16, pb[2]), PACKED_POISON, dtype=np.uint8)
        ctx.h2d(dA, A.view(np.uint8)); ctx.h2d(dB, B.view(np.uint8))
        on.pack(capi.OPERAND_A, dA, pA, strides[0], ld[0])
        on.pack(capi.OPERAND_B, dB, pB, strides[1], ld[1])
        out = []
        for plan in (on, off):
            ctx.h2d(dC, C.view(np.uint8)); ctx.h2d(pC, raw)
            if timed and plan is on:
                assert plan.time_execute(pC, pA, pB, 1, 2) > 0
            else:
                plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC, strides[2], ld[2])
            ctx.sync()
            got = C.copy()
            ctx.d2h(got.view(np.uint8), dC)
            out.append(got)
            if packed_c is not None and plan is on:
                p = raw.copy()
                ctx.d2h(p, pC)
                packed_c.append(p)
        return out[0], out[1], on.launches, off.launches
    finally:
        for p in bufs:
            ctx.free(p)
        on.close()
        off.close()


def check(ctx, oracle, d, e, ec, batches, flags=0, seed=1000, one_launch=True):
    """members of max(batches) generated once; oracle == plain plan == unflagged batched plan == flagged batched plan for every batch count"""
    nb = max(batches)
    extA, extB, extC = extents(d)
    strides = (extA + 3, extB + 5, extC + 7)
    A, mA = host_batch(oracle, e, nb, extA, strides[0], seed, (0, 1))
    B, mB = host_batch(oracle, e, nb, extB, strides[1], seed + 500, (0, 1))
    exp = [oracle.gemm(d, a, b, ec, nthreads=8) for a, b in zip(mA, mB)]
    plain = run_plain_members(ctx, oracle, d, ec, mA, mB) if not flags else None   # (a case with plan flags: plain_with_flags)
    for b in range(nb if plain else 0):
        assert plain[b].tobytes() == exp[b].tobytes(), ("plain plan", b)
    for batch in batches:
        on, off, n_on, n_off = run_both(ctx, oracle, d, ec, batch, A[:(batch - 1) * strides[0] + extA], B[:(batch - 1) * strides[1] + extB], strides, flags=flags, one_launch=one_launch)
        want = expected_buffer(oracle, d, ec, batch, exp, strides[2]).tobytes()
        assert off.tobytes() == want, ("unflagged", batch)
        assert on.tobytes() == want, ("flagged", batch)
        assert n_on == (1 if one_launch else n_off), (batch, n_on, n_off)
    return exp


# ---- a. every step form of the four kernels
@pytest.mark.parametrize("case", [c for c in REAL if c[4] == "tree_i32"], ids=lambda c: c[5].replace(" ", "_"))
def test_every_real_step_form(ctx, oracle, case):
    """M = 70, N = 41: two row tiles of the 64-row kernels, both partial in N; K = 40 pads to 64 leaves"""
    e, ec, kw, flags, kernel, form = case
    d = lower(e, e, ec, 70, 41, 40, **kw)
    planned(d, 3, flags, form, kernel)
    check(ctx, oracle, d, e, ec, (3,), flags=flags)
    if flags:   # (the plain plan of a flagged case: through the flag-aware parity helper's plan)
        plain_with_flags(ctx, oracle, d, e, ec, flags)


@pytest.mark.parametrize("case", CPLX, ids=lambda c: c[4].replace(" ", "_"))
def test_every_complex_step_form(ctx, oracle, case):
    e, ec, kw, flags, form = case
    d = lower(e, e, ec, 33, 29, 40, **kw)
    planned(d, 3, flags, form, "tree_cplx_i32")
    check(ctx, oracle, d, e, ec, (3,), flags=flags)
    if flags:
        plain_with_flags(ctx, oracle, d, e, ec, flags)


def plain_with_flags(ctx, oracle, d, e, ec, flags):
    """one member through a PLAIN plan created with `flags` == the oracle (the member kernel the flagged batch's twin mirrors)"""
    extA, extB, extC = extents(d)
    a, b = oracle.fill(e, extA, 1000, 0), oracle.fill(e, extB, 1500, 0)
    plan = capi.Plan(ctx, d, flags)
    pb = plan.info.packed_bytes
    bufs = [ctx.alloc(a.nbytes), ctx.alloc(b.nbytes), ctx.alloc(extC * plan.info.host_elem_bytes[2]), ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])]
    dA, dB, dC, pA, pB, pC = bufs
    try:
        ctx.h2d(dA, a.view(np.uint8)); ctx.h2d(dB, b.view(np.uint8))
        plan.pack(capi.OPERAND_A, dA, pA, 0)
        plan.pack(capi.OPERAND_B, dB, pB, 0)
        plan.execute(pC, pA, pB)
        plan.unpack_c(pC, dC, 0)
        ctx.sync()
        c = np.zeros(extC, dtype=oracle.host_dtype(ec))
        ctx.d2h(c.view(np.uint8), dC)
        assert c.tobytes() == oracle.gemm(d, a, b, ec, nthreads=8).tobytes()
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


# ---- b. shapes and batch counts
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("name", sorted(MEMBERS))
def test_shapes_and_batch_counts(ctx, oracle, name, shape):
    e, kw, kernel, form = MEMBERS[name]
    M, N, K = shape
    d = lower(e, e, e, M, N, K, **kw)
    # (one output column of a real member belongs to the one-column kernel, which has no twin: member by member under the flag too)
    one_launch = not (N == 1 and not d.is_complex)
    if one_launch:
        for batch in BATCHES:
            planned(d, batch, 0, form, kernel)
    else:
        assert capi.KERNEL_NAMES[capi.classify(d).kernel] == "gemv_i32" and capi.classify_batched_launches(d, 9, F) == 9
    exp = check(ctx, oracle, d, e, e, BATCHES, seed=2000, one_launch=one_launch)
    if K > 1:
        assert len({x.tobytes() for x in exp}) > 1


# ---- c. more than one group of 16 tile rows inside a member, the last group short
def test_group_walk_inside_a_member(ctx, oracle):
    d = lower(E88, E88, E88, 1089, 33, 32)   # 18 x 2 tiles
    planned(d, 3, 0, "left-justified", "tree_i32")
    check(ctx, oracle, d, E88, E88, (3,), seed=3000)


# ---- d. strides, leading dimensions, poison between the members: in the host C and in the packed C
@pytest.mark.parametrize("name", ["e88_lj", "c5_tf"])
def test_strides_leading_dimensions_and_poison(ctx, oracle, name):
    e, kw, kernel, form = MEMBERS[name]
    M, N, K, batch = 65, 33, 40, 3
    d = lower(e, e, e, M, N, K, **kw)
    planned(d, batch, 0, form, kernel)
    ld = (M + 3, K + 5, M + 7)
    extA, extB, extC = extents(d, *ld)
    strides = (extA + 11, extB + 1, extC + 13)
    A, mA = host_batch(oracle, e, batch, extA, strides[0], 700, (0,))
    B, mB = host_batch(oracle, e, batch, extB, strides[1], 800, (0,))
    packed = []
    on, off, n_on, n_off = run_both(ctx, oracle, d, e, batch, A, B, strides, ld, packed_c=packed)
    assert (n_on, n_off) == (1, batch)
    exp = []
    for a, b in zip(mA, mB):
        out = np.zeros(extC, dtype=oracle.host_dtype(e))
        oracle.gemm(d, a, b, e, lda=ld[0], ldb=ld[1], ldc=ld[2], out=out, nthreads=8)
        exp.append(np.concatenate([out[j * ld[2]:j * ld[2] + M] for j in range(N)]))
    want = expected_buffer(oracle, d, e, batch, exp, strides[2], ld[2]).tobytes()
    assert on.tobytes() == want and off.tobytes() == want
    # the packed C: a member's M N containers per part, then poison up to the next member's start (a multiple of 256 bytes)
    info = capi.classify_batched_status(d, batch, F)[1]
    step = info.packed_bytes[2] // batch
    used = capi.classify(d).packed_bytes[2]   # (the plain plan's packed C: [parts][M][N] containers)
    assert step % 256 == 0 and 0 < used < step
    for b in range(batch):
        member = packed[0][b * step:(b + 1) * step]
        assert (member[used:] == PACKED_POISON).all(), b
        assert not (member[:used] == PACKED_POISON).all(), b


# ---- e. more workgroups than CUs
def test_more_workgroups_than_cus(ctx, oracle):
    e, kw, kernel, form = MEMBERS["e43_pk16"]
    d = lower(e, e, e, 64, 64, 64, **kw)
    batch, n = 600, 64 * 64
    planned(d, batch, 0, form, kernel)
    A, mA = host_batch(oracle, e, batch, n, n, 300, (0, 1))
    B, mB = host_batch(oracle, e, batch, n, n, 400, (0, 1))
    on, off, n_on, n_off = run_both(ctx, oracle, d, e, batch, A, B, (n, n, n))
    assert (n_on, n_off) == (1, batch)
    plain = run_plain_members(ctx, oracle, d, e, mA, mB)
    assert on.tobytes() == np.concatenate(plain).tobytes() == off.tobytes()
    for i in (0, batch // 2, batch - 1):
        assert oracle.gemm(d, mA[i], mB[i], e, nthreads=8).tobytes() == on[i * n:(i + 1) * n].tobytes(), i


# ---- f. what the flag leaves member by member, through the same entry
FALLBACKS = {
    # name -> (element, C element, lowering keywords, shape, kernel)
    "13_levels": (E88, E88, {}, (17, 9, 4097), "tree_i32"),
    "one_column": (E88, E88, {}, (33, 1, 40), "gemv_i32"),
    "tree_i64": (REAL[-1][0], REAL[-1][1], REAL[-1][2], (33, 17, 40), "tree_i64"),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallbacks_under_the_flag_run_member_by_member(ctx, oracle, name):
    e, ec, kw, (M, N, K), kernel = FALLBACKS[name]
    batch = 3
    d = lower(e, e, ec, M, N, K, **kw)
    st, info = capi.classify_batched_status(d, batch, F)
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == kernel and "in one launch" not in reason(info)
    assert capi.classify_batched_launches(d, batch, F) == batch == capi.classify_batched_launches(d, batch)
    check(ctx, oracle, d, e, ec, (batch,), seed=4000, one_launch=False)


def test_a_mixed_member_is_refused_under_the_flag_as_without(ctx):
    d = lower(E43, C5, Qcomplex(Qu(14, 3), Qu(14, 3)), 33, 17, 40)
    for flags in (0, F):
        assert capi.classify_batched_status(d, 3, flags)[0] == capi.QG_EUNSUPPORTED
        with pytest.raises(capi.QgemulError):
            capi.BatchedPlan(ctx, d, 3, flags)


# ---- g. the other entry points
def test_time_execute_batched_leaves_the_right_c(ctx, oracle):
    e, kw, kernel, form = MEMBERS["e88_lj"]
    d = lower(e, e, e, 65, 33, 40, **kw)
    extA, extB, extC = extents(d)
    A, mA = host_batch(oracle, e, 7, extA, extA, 5000, (0, 1))
    B, mB = host_batch(oracle, e, 7, extB, extB, 5500, (0, 1))
    on, off, n_on, _ = run_both(ctx, oracle, d, e, 7, A, B, (extA, extB, extC), timed=True)
    exp = np.concatenate([oracle.gemm(d, a, b, e, nthreads=8) for a, b in zip(mA, mB)])
    assert n_on == 1 and on.tobytes() == exp.tobytes() == off.tobytes()


@pytest.mark.parametrize("name", ["e88_lj", "c5_tf"])
def test_one_shot_call_and_replanning_when_the_flag_toggles(ctx, oracle, name):
    e, kw, kernel, form = MEMBERS[name]
    M, N, K, batch = 65, 33, 40, 7
    d = lower(e, e, e, M, N, K, **kw)
    extA, extB, extC = extents(d)
    strides = (extC + 9, extA + 1, extB + 2)                                  # (C, A, B: the order of qgemul_run_batched)
    A, mA = host_batch(oracle, e, batch, extA, strides[1], 40, (0, 1))
    B, mB = host_batch(oracle, e, batch, extB, strides[2], 50, (0, 1))
    exp = [oracle.gemm(d, a, b, e, nthreads=8) for a, b in zip(mA, mB)]
    want = expected_buffer(oracle, d, e, batch, exp, strides[0]).tobytes()
    on, off, _, _ = run_both(ctx, oracle, d, e, batch, A, B, (strides[1], strides[2], strides[0]))
    assert on.tobytes() == want == off.tobytes()
    try:
        for flags in (F, 0, 0, F, F):
            out = np.empty((batch - 1) * strides[0] + extC, dtype=oracle.host_dtype(e))
            out.view(np.uint8)[:] = POISON
            capi.run_batched(d, batch, out, A, B, *strides, flags=flags)
            assert out.tobytes() == want, flags
    finally:
        capi.run_release()


# ---- h. the drop-in program: QgemulBatched on 3-d tensors with QgemulRunFlags() |= QG_OPT_BATCHED_TREE
@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_runs_tree_batches_in_one_launch(oracle, tmp_path):
    exe = tmp_path / "amd_header_batched_tree_run"
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++23", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "binding", "amd_header_batched_tree_run.cpp"),
                           "-o", str(exe), "-L" + lib, "-lqugemm", "-Wl,-rpath," + lib])
    recs = [json.loads(l) for l in subprocess.check_output([str(exe)], text=True).splitlines() if l.strip()]
    assert "error" not in str(recs) and [(r["name"], r["flagged"]) for r in recs] == [("e88_default", 0), ("c5_tf", 0), ("e88_default", 1), ("c5_tf", 1)]
    M, N, K, Bt = 70, 41, 40, 5
    real = lambda n, mul, add: np.array([(i * mul + add) % 8192 - 4096 for i in range(n)], dtype=np.int32)

    def cplx(n, mul):
        h = np.zeros(n, dtype=oracle.host_dtype(C5))
        h["re"] = [(i * mul + 7) % 1024 - 512 for i in range(n)]
        h["im"] = [(i * 40503 + 3) % 16 - 8 for i in range(n)]
        return h
    calls = {"e88_default": (lower(E88, E88, E88, M, N, K), real(M * K * Bt, 37, 0), real(K * N * Bt, 53, 1), E88),
             "c5_tf": (lower(C5, C5, C5, M, N, K, mul_args=TFComplexMul()), cplx(M * K * Bt, 53), cplx(K * N * Bt, 29), C5)}
    for name, (d, A, B, ec) in calls.items():
        plain, flagged = [r for r in recs if r["name"] == name]
        assert plain["launches"] == Bt == capi.classify_batched_launches(d, Bt) and flagged["launches"] == 1 == capi.classify_batched_launches(d, Bt, F), name
        assert flagged["C"] == plain["C"], name
        exp = np.concatenate([oracle.gemm(d, A[b * M * K:(b + 1) * M * K], B[b * K * N:(b + 1) * K * N], ec, nthreads=8) for b in range(Bt)])
        got = np.asarray(flagged["C"], dtype=np.int64)
        if d.is_complex:
            assert np.array_equal(got[0::2], exp["re"].astype(np.int64)) and np.array_equal(got[1::2], exp["im"].astype(np.int64)), name
        else:
            assert np.array_equal(got, exp.astype(np.int64)), name
        assert len(set(flagged["C"])) > 20
