"""Element-wise chains on batched plans, on the GPU (run with -m gpu): member b is Qgemul<...>(C_b, A_b, B_b) followed by the chain.
Every case is compared member by member with the oracle (oracle.gemm, then oracle.eltwise for the plain stages and the
restatement tests/approx_ref.py for an APPROX stage) AND byte for byte with qgemul_execute_ep of that member through a plain plan
with the same chain.  The three forms — chain fused into the block-diagonal launch, one block-diagonal pass behind it, member by
member — are asked for by flag and checked through qgemul_plan_fuses_epilogue and qgemul_plan_batched_launches.  Shapes: one ragged
tile, 2 x 1 and 3 x 3 tiles per member, batches 1, 2 and 9, 300 members of one tile; host buffers carry poison between members."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import batched_ep_cases as X
from qublas_amd import capi
from qublas_amd.desc import Approx, Ew, Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, lower, lower_epilogue, lower_epilogue_x

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FUSED, UNFUSED = capi.OPT_FUSED_EPILOGUE, capi.OPT_UNFUSED_EPILOGUE
POISON = X.POISON


@pytest.fixture(scope="module")
def ctx():
    with capi.Context() as c:
        yield c


class Operands:
    """the stage operands of one case for `batch` members: per stage a list of member tensors (one entry when shared), a scalar or
    None (APPROX); host buffers with poison between the members of a per-member operand"""

    def __init__(self, oracle, stages, shared, n, batch, seed0=170, gap=0):
        self.stages, self.shared, self.n, self.gap = stages, shared, n, gap
        self.members, self.host, self.stride = [], [], []
        for k, st in enumerate(stages):
            if isinstance(st, Approx):
                self.members.append(None); self.host.append(None); self.stride.append(0)
            elif st.scalar:
                h = oracle.fill(st.e, 1, seed0 + k, 0)
                self.members.append([h]); self.host.append(h); self.stride.append(0)
            elif shared[k]:
                h = oracle.fill(st.e, n, seed0 + k, 0)
                self.members.append([h]); self.host.append(h); self.stride.append(0)
            else:
                buf, mem = X.host_batch(oracle, st.e, batch, n, n + gap, seed0 + 100 * k, (0,))
                self.members.append(mem); self.host.append(buf); self.stride.append(n + gap)

    def of_member(self, b):
        """the oracle's view (int64) and the host arrays of member b's operands"""
        Eo, Eh = [], []
        for k, m in enumerate(self.members):
            h = None if m is None else m[b if len(m) > 1 else 0]
            Eh.append(h)
            Eo.append(None if h is None else h.astype(np.int64))
        return Eo, Eh


def run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A, B, ops, strides, flags=0, ld=(0, 0, 0), shared=None, eld=0):
    """pack_batched, pack_e_batched, execute_batched_ep, unpack_c_batched into a poisoned D; returns (D buffer, fuses, launches)"""
    shared = ops.shared if shared is None else shared
    extD = X.extents(d, *ld)[2]
    D = np.empty((batch - 1) * strides[2] + extD, dtype=oracle.host_dtype(dq))
    D.view(np.uint8)[:] = POISON
    plan = capi.BatchedPlan(ctx, d, batch, flags, ep=ep, approx=tabs, shared=shared)
    pb = plan.info.packed_bytes
    assert plan.info.host_elem_bytes[2] == D.dtype.itemsize
    bufs = [ctx.alloc(max(16, A.nbytes)), ctx.alloc(max(16, B.nbytes)), ctx.alloc(max(16, D.nbytes)), ctx.alloc(max(16, pb[0])), ctx.alloc(max(16, pb[1])), ctx.alloc(max(16, pb[2]))]
    dA, dB, dD, pA, pB, pD = bufs
    try:
        ctx.h2d(dA, A.view(np.uint8)); ctx.h2d(dB, B.view(np.uint8)); ctx.h2d(dD, D.view(np.uint8))
        plan.pack(capi.OPERAND_A, dA, pA, strides[0], ld[0])
        plan.pack(capi.OPERAND_B, dB, pB, strides[1], ld[1])
        packed, scalars = [0] * len(ops.stages), [0] * len(ops.stages)
        for k, st in enumerate(ops.stages):
            if isinstance(st, Approx):
                assert plan.packed_e_bytes(k) == 0
            elif st.scalar:
                assert plan.packed_e_bytes(k) == 0
                scalars[k] = int(ops.host[k][0])
            else:
                dE, pE = ctx.alloc(ops.host[k].nbytes), ctx.alloc(plan.packed_e_bytes(k))
                bufs += [dE, pE]
                ctx.h2d(dE, ops.host[k].view(np.uint8))
                plan.pack_e(k, dE, pE, 0 if shared[k] else ops.stride[k], eld)
                packed[k] = pE
        plan.execute_ep(pD, pA, pB, capi.Plan.ep_args(packed=packed, scalars=scalars))
        plan.unpack_c(pD, dD, strides[2], ld[2])
        ctx.sync()
        ctx.d2h(D.view(np.uint8), dD)
        return D, plan.fuses, plan.launches
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


def run_plain_members(ctx, oracle, d, ep, tabs, dq, membersA, membersB, ops, which, ld=(0, 0, 0)):
    """members `which` through a PLAIN plan with the same chain: qgemul_pack, qgemul_pack_e, qgemul_execute_ep, qgemul_unpack_c"""
    plan = capi.Plan(ctx, d, epilogue=ep, approx=tabs)
    pb = plan.info.packed_bytes
    n = d.M * d.N
    out = []
    bufs = [ctx.alloc(max(16, membersA[0].nbytes)), ctx.alloc(max(16, membersB[0].nbytes)), ctx.alloc(max(16, n * plan.info.host_elem_bytes[2])),
            ctx.alloc(max(16, pb[0])), ctx.alloc(max(16, pb[1])), ctx.alloc(max(16, pb[2]))]
    dA, dB, dD, pA, pB, pD = bufs
    pe = {}
    for k, st in enumerate(ops.stages):
        if not isinstance(st, Approx) and not st.scalar:
            pe[k] = (ctx.alloc(n * np.dtype(oracle.host_dtype(st.e)).itemsize), ctx.alloc(plan.packed_e_bytes(k)))
            bufs += list(pe[k])
    try:
        for b in which:
            _, Eh = ops.of_member(b)
            ctx.h2d(dA, membersA[b].view(np.uint8)); ctx.h2d(dB, membersB[b].view(np.uint8))
            plan.pack(capi.OPERAND_A, dA, pA, ld[0])
            plan.pack(capi.OPERAND_B, dB, pB, ld[1])
            packed, scalars = [0] * len(ops.stages), [0] * len(ops.stages)
            for k, st in enumerate(ops.stages):
                if isinstance(st, Approx):
                    continue
                if st.scalar:
                    scalars[k] = int(Eh[k][0])
                else:
                    ctx.h2d(pe[k][0], Eh[k].view(np.uint8))
                    plan.pack_e(k, pe[k][0], pe[k][1])
                    packed[k] = pe[k][1]
            plan.execute_ep(pD, pA, pB, capi.Plan.ep_args(packed=packed, scalars=scalars))
            plan.unpack_c(pD, dD, 0)
            ctx.sync()
            c = np.zeros(n, dtype=oracle.host_dtype(dq))
            ctx.d2h(c.view(np.uint8), dD)
            out.append(c)
        return out
    finally:
        for p in bufs:
            ctx.free(p)
        plan.close()


def expected_buffer(oracle, d, dq, batch, membersD, stride, ldc=0):
    """what the batched D buffer must hold: the members at their stride (columns at ldc), poison everywhere else"""
    ext = (d.N - 1) * (ldc or d.M) + d.M
    exp = np.empty((batch - 1) * stride + ext, dtype=oracle.host_dtype(dq))
    exp.view(np.uint8)[:] = POISON
    for b in range(batch):
        for j in range(d.N):
            o = b * stride + j * (ldc or d.M)
            exp[o:o + d.M] = membersD[b][j * d.M:(j + 1) * d.M]
    return exp


def oracle_members(oracle, d, ec, stages, dq, mA, mB, ops, nthreads=8):
    out = []
    for b, (a, bb) in enumerate(zip(mA, mB)):
        Cx = oracle.gemm(d, a, bb, ec, nthreads=nthreads).astype(np.int64)
        out.append(X.expected(oracle, ec, stages, dq, Cx, ops.of_member(b)[0]).astype(oracle.host_dtype(dq)))
    return out


# which rows run which chain: every row runs chain 1; the others once per geometry that matters for them
CASES = ([(f, "1_scale_shared_bias") for f in sorted(X.FORMATS)] +
         [(f, c) for f in ("e43_c1byte", "e88_3x3", "q78_centred") for c in ("2_member_sub_shared_mul_wide", "4_four_stages_1_2_4_8_bytes")] +
         [(f, "3_no_stage_narrow_sat") for f in ("e43_c1byte", "e88_3x3", "e88_x_e43_3x1_c16", "e88_3x3_tn_c16")] +
         [(f, c) for f in ("e43_c1byte", "e88_3x3_c16") for c in ("5_act_uniform", "5_act_general", "5_act_member_operand")] +
         # k_approx_bd's remaining branches: 32-bit with a scalar and a SHARED operand, 64-bit with per-member operands only
         [("e43_c1byte", "6_act_scalar_32bit"), ("e88_3x3_c16", "6_act_scalar_32bit"), ("e88_3x3_c16", "6_act_member_operand_wide")])


@pytest.mark.parametrize("shape", X.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("fmt,chain", CASES, ids=lambda v: v)
def test_chain_forms_vs_oracle_and_plain_plan(ctx, oracle, fmt, chain, shape):
    d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, shape, chain)
    extA, extB, extD = X.extents(d)
    nb = max(X.BATCHES)
    A, mA = X.host_batch(oracle, X.FORMATS[fmt][0], nb, extA, extA, 100, (0, 1))
    B, mB = X.host_batch(oracle, X.FORMATS[fmt][1], nb, extB, extB, 200, (0, 1))
    ops = Operands(oracle, stages, shared, extD, nb)
    exp = oracle_members(oracle, d, ec, stages, dq, mA, mB, ops)                       # computed once, shared by every batch and form
    plain = run_plain_members(ctx, oracle, d, ep, tabs, dq, mA, mB, ops, range(nb))
    for b in range(nb):
        assert plain[b].tobytes() == exp[b].tobytes(), (fmt, chain, shape, b)
    fusable = X.bits32(d, ep, tabs) and not X.has_approx(stages)
    if chain == "1_scale_shared_bias":
        assert fusable == (fmt == "e43_c1byte" or fmt.endswith("_c16")), fmt          # (32-bit chain wherever C has at most 32 storage bits)
    if chain.startswith("6_"):
        assert X.bits32(d, ep, tabs) == chain.endswith("_32bit") and not fusable
    if chain.startswith(("2_", "4_", "5_")):
        assert not fusable or chain == "5_act_member_operand"
    for batch in X.BATCHES:
        got = {}
        for flags in (0, FUSED, UNFUSED):
            D, fuses, launches = run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A[:batch * extA], B[:batch * extB], ops, (extA, extB, extD), flags)
            want_fused = X.fused_expected(fusable, flags)
            assert (fuses, launches) == ((1, 1) if want_fused else (0, 2)), (fmt, chain, shape, batch, flags)
            assert D.tobytes() == expected_buffer(oracle, d, dq, batch, exp, extD).tobytes(), (fmt, chain, shape, batch, flags)
            got[flags] = D
        assert got[FUSED].tobytes() == got[UNFUSED].tobytes() == got[0].tobytes()


@pytest.mark.parametrize("fmt", ["e43_c1byte", "e88_3x3_c16", "e88_3x3"])
def test_shared_operand_equals_the_same_operand_given_per_member(ctx, oracle, fmt):
    """random operands, 2 tiles per member: a wrong member offset cannot pass this together with the oracle comparison"""
    d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, (65, 33, 100), "1_scale_shared_bias")
    batch = 9
    extA, extB, extD = X.extents(d)
    A, mA = X.host_batch(oracle, X.FORMATS[fmt][0], batch, extA, extA, 100, (0, 1))
    B, mB = X.host_batch(oracle, X.FORMATS[fmt][1], batch, extB, extB, 200, (0, 1))
    ops = Operands(oracle, stages, shared, extD, batch)
    copies = Operands(oracle, stages, [0, 0], extD, batch)
    copies.members[1] = [ops.members[1][0]] * batch
    copies.host[1] = np.concatenate(copies.members[1])
    copies.stride[1] = extD
    exp = oracle_members(oracle, d, ec, stages, dq, mA, mB, ops)
    assert len({e.tobytes() for e in exp}) == batch
    for flags in (FUSED, UNFUSED):
        one, f1, _ = run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A, B, ops, (extA, extB, extD), flags)
        many, f2, _ = run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A, B, copies, (extA, extB, extD), flags)
        assert f1 == f2 == (1 if flags == FUSED and fmt != "e88_3x3" else 0)
        assert one.tobytes() == many.tobytes() == np.concatenate(exp).tobytes(), (fmt, flags)


@pytest.mark.parametrize("fmt,chain", [("e43_c1byte", "1_scale_shared_bias"), ("e88_3x3_tn_c16", "1_scale_shared_bias"), ("q78_centred_c16", "5_act_member_operand"),
                                       ("e88_3x3_tn", "4_four_stages_1_2_4_8_bytes")], ids=lambda v: v)
def test_strides_and_leading_dimensions_with_poison(ctx, oracle, fmt, chain):
    """poison between members and between columns of A, B, per-member E and D; D's gaps survive"""
    d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, (65, 33, 100), chain)
    M, N, K, batch = 65, 33, 100, 3
    ta = bool(d.transA)
    ld = ((K if ta else M) + 3, K + 5, M + 7)
    eld = M + 4
    extA, extB, extD = X.extents(d, *ld)
    extE = (N - 1) * eld + M
    strides = (extA + 11, extB + 1, extD + 13)
    A, mA = X.host_batch(oracle, X.FORMATS[fmt][0], batch, extA, strides[0], 700, (0,))
    B, mB = X.host_batch(oracle, X.FORMATS[fmt][1], batch, extB, strides[1], 800, (0,))
    ops = Operands(oracle, stages, shared, extE, batch, gap=6)                            # operand tensors at leading dimension eld
    exp = []
    tight = lambda v, l: np.concatenate([v[j * l:j * l + M] for j in range(N)])
    for b, (a, bb) in enumerate(zip(mA, mB)):
        out = np.zeros(extD, dtype=oracle.host_dtype(ec))
        oracle.gemm(d, a, bb, ec, lda=ld[0], ldb=ld[1], ldc=ld[2], out=out, nthreads=8)
        Eo = [None if e is None else (e if e.size == 1 else tight(e, eld)) for e in ops.of_member(b)[0]]
        exp.append(X.expected(oracle, ec, stages, dq, tight(out, ld[2]).astype(np.int64), Eo).astype(oracle.host_dtype(dq)))
    for flags in (FUSED, UNFUSED):
        D, _, launches = run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A, B, ops, strides, flags, ld, eld=eld)
        assert launches == (1 if flags == FUSED and chain.startswith("1_") else 2)
        assert D.tobytes() == expected_buffer(oracle, d, dq, batch, exp, strides[2], ld[2]).tobytes(), (fmt, flags)


@pytest.mark.parametrize("fmt", ["e43_c1byte", "e88_3x3_c16"])
def test_more_workgroups_than_cus(ctx, oracle, fmt):
    d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, (64, 64, 64), "1_scale_shared_bias")
    batch, n = 300, 64 * 64
    A, mA = X.host_batch(oracle, X.FORMATS[fmt][0], batch, n, n, 300, (0, 1))
    B, mB = X.host_batch(oracle, X.FORMATS[fmt][1], batch, n, n, 400, (0, 1))
    ops = Operands(oracle, stages, shared, n, batch)
    exp = np.concatenate(oracle_members(oracle, d, ec, stages, dq, mA, mB, ops))
    sample = [0, 1, 7, 8, 150, 299]
    plain = run_plain_members(ctx, oracle, d, ep, tabs, dq, mA, mB, ops, sample)
    for flags, form in ((FUSED, (1, 1)), (UNFUSED, (0, 2))):
        D, fuses, launches = run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A, B, ops, (n, n, n), flags)
        assert (fuses, launches) == form
        assert D.tobytes() == exp.tobytes(), (fmt, flags)
        for i, c in zip(sample, plain):
            assert c.tobytes() == D[i * n:(i + 1) * n].tobytes(), (fmt, flags, i)


@pytest.mark.parametrize("dists", [(1, 0), (0, 1), (1, 1)], ids=["small_then_full_range", "full_range_then_small", "all_small"])
def test_stack_wide_plane_mask_with_a_fused_chain(ctx, oracle, dists):
    """int<8,8> in three limb planes, fused: ONE plane mask for the stack decides which kernel of the launch pair stores D, so both
    partners carry the chain (all members small: the 2 x 2 partner; a full-range member anywhere: the 3 x 3 kernel)"""
    fmt = "e88_3x3_c16"
    d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, (65, 33, 100), "1_scale_shared_bias")
    batch = 2
    extA, extB, extD = X.extents(d)
    A, mA = X.host_batch(oracle, X.E88, batch, extA, extA + 5, 500, dists)
    B, mB = X.host_batch(oracle, X.E88, batch, extB, extB + 3, 600, dists)
    ops = Operands(oracle, stages, shared, extD, batch)
    exp = oracle_members(oracle, d, ec, stages, dq, mA, mB, ops)
    D, fuses, launches = run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A, B, ops, (extA + 5, extB + 3, extD), FUSED)
    assert (fuses, launches) == (1, 1)
    assert D.tobytes() == np.concatenate(exp).tobytes(), dists
    assert len(set(D.tolist())) > 100


C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
I16 = Qu(15, 0, True, TRN.TCPL, WRP.TCPL)
# the real fallback kinds of tests/test_gpu_batched.py, by value: (operand element, C element, lowering keywords, class)
FALLBACKS = {
    "tree_default_tags": (X.E88, X.E88, {}, 2),
    "ring_int16": (I16, I16, {}, 1),
    "raw_pass_left_shift": (Qu(10, -3), Qu(24, 9), dict(mul_args=Tags(21, -6), add_args=[Qu(28, -6)]), 1),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallback_kinds_run_member_by_member(ctx, oracle, name):
    e, ec, kw, cls = FALLBACKS[name]
    M, N, K, batch = 33, 17, 40, 3
    d = lower(e, e, ec, M, N, K, **kw)
    stages = [Ew("mul", X.S34, scalar=True, into=ec), Ew("add", X.B106, into=ec), Ew("sub", X.B106)]
    shared, dq = [0, 1, 0], ec
    ep, tabs = lower_epilogue_x(ec, stages, dq)
    st, info = capi.classify_batched_epx_status(d, batch, ep, tabs, shared)
    assert st == capi.QG_OK and info.cls == cls and b"member by member" in bytes(info.reason), info.reason
    extA, extB, extD = X.extents(d)
    strides = (extA + 2, extB + 3, extD + 4)
    A, mA = X.host_batch(oracle, e, batch, extA, strides[0], 900, (1,))
    B, mB = X.host_batch(oracle, e, batch, extB, strides[1], 950, (1,))
    ops = Operands(oracle, stages, shared, extD, batch, gap=5)
    exp = oracle_members(oracle, d, ec, stages, dq, mA, mB, ops, nthreads=4)
    one = capi.Plan(ctx, d, epilogue=ep)                       # what one member's qgemul_execute_ep issues: its kernel(s) and the chain's pass
    per_member = (2 if name == "raw_pass_left_shift" else 1) + (0 if one.fuses_epilogue() else 1)
    one.close()
    D, _, launches = run_batched_ep(ctx, oracle, d, ep, tabs, dq, batch, A, B, ops, strides)
    assert launches == batch * per_member == capi.classify_batched_epx_launches(d, batch, ep, tabs, shared)
    assert D.tobytes() == expected_buffer(oracle, d, dq, batch, exp, strides[2]).tobytes()


def test_entry_points_refuse_each_other(ctx):
    d, ep, tabs, stages, ec, dq, shared = X.lowered("e43_c1byte", (64, 64, 64), "1_scale_shared_bias")
    bep = capi.BatchedPlan(ctx, d, 2, ep=ep, shared=shared)
    bp, pp, pep = capi.BatchedPlan(ctx, d, 2), capi.Plan(ctx, d), capi.Plan(ctx, d, epilogue=ep)
    buf = ctx.alloc(1 << 16)
    L, v = capi.lib(), C.c_void_p
    args = capi.Plan.ep_args(packed=[0, buf], scalars=[3, 0])
    ms = C.c_float()
    EINVAL = capi.QG_EINVAL
    try:
        # the plain entry points refuse the batched plan with a chain
        assert L.qgemul_execute(bep.h, v(buf), v(buf), v(buf)) == EINVAL
        assert L.qgemul_execute_ep(bep.h, v(buf), v(buf), v(buf), C.byref(args)) == EINVAL
        assert L.qgemul_pack(bep.h, 0, v(buf), 0, v(buf)) == EINVAL
        assert L.qgemul_pack_e(bep.h, 1, v(buf), 0, v(buf)) == EINVAL
        assert L.qgemul_pack_c(bep.h, v(buf), 0, v(buf)) == EINVAL
        assert L.qgemul_apply_epilogue(bep.h, v(buf), v(buf), C.byref(args)) == EINVAL
        assert L.qgemul_unpack_c(bep.h, v(buf), v(buf), 0) == EINVAL
        assert L.qgemul_time_execute_ep(bep.h, v(buf), v(buf), v(buf), C.byref(args), 0, 1, C.byref(ms)) == EINVAL
        assert L.qgemul_export_bitstream(bep.h, v(buf), 0, 0, 0, v(buf)) == EINVAL
        # qgemul_execute_batched treats it as qgemul_execute treats a plain plan with an epilogue
        assert L.qgemul_execute(pep.h, v(buf), v(buf), v(buf)) == EINVAL
        assert L.qgemul_execute_batched(bep.h, v(buf), v(buf), v(buf)) == EINVAL
        assert L.qgemul_time_execute_batched(bep.h, v(buf), v(buf), v(buf), 0, 1, C.byref(ms)) == EINVAL
        # the _batched_ep entries refuse a batched plan without a chain and plain plans
        for h in (bp.h, pp.h, pep.h):
            assert L.qgemul_execute_batched_ep(h, v(buf), v(buf), v(buf), C.byref(args)) == EINVAL
            assert L.qgemul_pack_e_batched(h, 1, v(buf), 0, 0, v(buf)) == EINVAL
            assert L.qgemul_time_execute_batched_ep(h, v(buf), v(buf), v(buf), C.byref(args), 0, 1, C.byref(ms)) == EINVAL
        # strides of qgemul_pack_e_batched: shared exactly 0, a scalar stage never; a missing tensor operand
        assert L.qgemul_pack_e_batched(bep.h, 1, v(buf), 0, 4096, v(buf)) == EINVAL
        assert L.qgemul_pack_e_batched(bep.h, 0, v(buf), 0, 0, v(buf)) == EINVAL
        assert L.qgemul_pack_e_batched(bep.h, 1, v(buf), 63, 0, v(buf)) == EINVAL
        none = capi.Plan.ep_args(packed=[0, 0], scalars=[3, 0])
        assert L.qgemul_execute_batched_ep(bep.h, v(buf), v(buf), v(buf), C.byref(none)) == EINVAL
        per = capi.BatchedPlan(ctx, d, 2, ep=ep, shared=[0, 0])
        assert L.qgemul_pack_e_batched(per.h, 1, v(buf), 0, 0, v(buf)) == EINVAL
        assert L.qgemul_pack_e_batched(per.h, 1, v(buf), 0, 4095, v(buf)) == EINVAL
        per.close()
        assert (bep.fuses, bep.launches) == ((1, 1) if X.fused_expected(True, 0) else (0, 2))
        assert bep.time_execute_ep(buf, buf + 16384, buf + 32768, capi.Plan.ep_args(packed=[0, buf + 49152], scalars=[3, 0]), 1, 2) > 0
    finally:
        ctx.free(buf)
        for p in (bep, bp, pp, pep):
            p.close()


def test_one_shot_replans_over_batch_count_and_shared_pattern(oracle):
    fmt = "q78_centred_c16"
    d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, (65, 33, 100), "1_scale_shared_bias")
    extA, extB, extD = X.extents(d)
    sD, sA, sB = extD + 9, extA + 1, extB + 2
    A, mA = X.host_batch(oracle, X.FORMATS[fmt][0], 7, extA, sA, 40, (0, 1))
    B, mB = X.host_batch(oracle, X.FORMATS[fmt][1], 7, extB, sB, 50, (0, 1))
    ops = Operands(oracle, stages, [0, 1], extD, 7)
    per = Operands(oracle, stages, [0, 0], extD, 7, gap=3)
    exp_shared = oracle_members(oracle, d, ec, stages, dq, mA, mB, ops)
    exp_per = oracle_members(oracle, d, ec, stages, dq, mA, mB, per)
    plain_ep = lower_epilogue(ec, stages, dq)
    try:
        for o, exp in ((ops, exp_shared), (per, exp_per), (ops, exp_shared)):              # the shared flag flips and flips back
            for batch in (7, 2, 2, 7):
                out = np.empty((batch - 1) * sD + extD, dtype=oracle.host_dtype(dq))
                out.view(np.uint8)[:] = POISON
                capi.run_batched_epx(d, batch, ep, tabs, out, A, B, o.host, sD, sA, sB, o.stride + [0] * (4 - len(o.stride)))
                assert out.tobytes() == expected_buffer(oracle, d, dq, batch, exp, sD).tobytes(), batch
                # a plain qgemul_run_ep in between: the thread's cache holds one plan, batched or not
                one = capi.run_ep(d, plain_ep, np.zeros(extD, dtype=oracle.host_dtype(dq)), mA[0], mB[0], o.of_member(0)[1])
                assert one.tobytes() == exp[0].tobytes()
        assert capi.run_batched_epx_status(d, 2, ep, tabs, out, A, B, ops.host, sD, sA, sB, [0, 0, 0, 0], flags=capi.OPT_ALL_DEVICES) == capi.QG_EUNSUPPORTED
    finally:
        capi.run_release()


def test_packed_e_bytes_one_member_when_shared_the_stack_when_not(ctx):
    for fmt, shape, tiles in (("e43_c1byte", (65, 33, 100), 2), ("e88_3x3", (129, 130, 65), 9)):
        d, ep, tabs, stages, ec, dq, _ = X.lowered(fmt, shape, "4_four_stages_1_2_4_8_bytes")
        batch = 9
        for shared in ([1, 0, 1, 0], [0, 1, 0, 1]):
            plan = capi.BatchedPlan(ctx, d, batch, ep=ep, approx=tabs, shared=shared)
            for k, ebytes in enumerate((1, 2, 4, 8)):
                member = tiles * 64 * 64 * ebytes                                       # whole 64 x 64 tiles in the operand's container
                assert plan.packed_e_bytes(k) == (member if shared[k] else batch * member), (fmt, shared, k)
            assert plan.packed_e_bytes(4) == 0 and plan.packed_e_bytes(-1) == 0
            assert plan.info.packed_bytes[2] == batch * tiles * 64 * 64 * 4 and plan.info.host_elem_bytes[2] == 4
            plan.close()
    # member by member: the member's bytes in 256-byte steps, shared or not
    e = X.E88
    d = lower(e, e, e, 33, 17, 40)
    ep, tabs = lower_epilogue_x(e, [Ew("add", X.B106), Ew("sub", X.S34)], e)
    plan = capi.BatchedPlan(ctx, d, 3, ep=ep, approx=tabs, shared=[1, 0])
    step = lambda ebytes: (33 * 17 * ebytes + 255) // 256 * 256                  # Qu<10,6> in a 4-byte container, Qu<3,4> in a 1-byte one
    assert (plan.packed_e_bytes(0), plan.packed_e_bytes(1)) == (step(4), 3 * step(1))
    plan.close()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_batched_chain_program(tmp_path, oracle):
    """tests/binding/amd_header_batched_ep_run.cpp: QgemulBatched<tags..., QgemulResult<CT>>(D, A, B, ThenMul(s), ThenAdd(shared Bias),
    ThenSub(per-member Res), ThenApprox<...>()) on 3-d tensors through include/QuBLAS_amd.h"""
    import approx_ref as R
    exe = tmp_path / "amd_header_batched_ep_run"
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++23", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "binding", "amd_header_batched_ep_run.cpp"), "-o", str(exe), "-L" + lib, "-lqugemm", "-Wl,-rpath," + lib])
    r = json.loads(subprocess.check_output([str(exe)], text=True).strip().splitlines()[-1])
    assert r.get("name") == "scale_bias_residual_sigmoid", r
    M, N, K, batch = r["M"], r["N"], r["K"], r["batch"]
    e88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
    ct, t1, dt = Qu(15, 8), Qu(24, 8), Qu(1, 10, True, RND.CONV, SAT.TCPL)
    x312, sigmoid = R.case_table(next(j for j in R.cases() if j["name"] == "uniform_sigmoid_8x_degree3"))
    d = lower(e88, e88, ct, M, N, K, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
    stages = [Ew("mul", X.S34, Tags(24, 8), scalar=True, into=t1), Ew("add", X.B106, into=t1), Ew("sub", X.B106, into=x312), Approx(sigmoid)]
    gen = lambda n, mul, add, mod, off: (((np.arange(n, dtype=np.uint64) * np.uint64(mul) + np.uint64(add)) % np.uint64(mod)).astype(np.int64) - off)
    A, B = gen(batch * M * K, 2654435761, 0, 128, 64).astype(np.int32), gen(batch * K * N, 40503, 7, 128, 64).astype(np.int32)
    bias, res = gen(M * N, 97, 0, 512, 256), gen(batch * M * N, 131, 5, 1024, 512)
    exp = []
    for b in range(batch):
        Cx = oracle.gemm(d, A[b * M * K:(b + 1) * M * K], B[b * K * N:(b + 1) * K * N], ct).astype(np.int64)
        exp.append(X.expected(oracle, ct, stages, dt, Cx, [np.asarray([13], dtype=np.int64), bias, res[b * M * N:(b + 1) * M * N], None]))
    assert r["D"] == np.concatenate(exp).astype(np.int64).tolist()
    assert len(set(r["D"])) > 20
