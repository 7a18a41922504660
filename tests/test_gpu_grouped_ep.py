"""Element-wise chains on grouped plans, on the GPU (run with -m gpu): member g is Qgemul<...>(C_g, A_g, B_g) followed by the group's
ONE chain, with that member's tensor operands and — for a per-member scalar stage — that member's raw scalar.

The comparison is always byte for byte, on poisoned D buffers (poison between the columns and behind every member):
oracle (oracle.gemm, then tests/batched_ep_cases.expected)  ==  a loop of plain _epx plans  ==  the grouped pass form  ==  the
grouped fused form where the chain is fusable.  The member shapes are the smallest at which the schedule, the tile -> member
table, the padding or the stragglers' offsets can go wrong: (64,64,1), (3,5,7), an empty (0,5,7), (16,200,64), (129,130,65),
(65,33,100), (1,1,300) in ASCENDING K — the schedule sorts by decreasing k-tile count, so its order differs from list order — plus
three members of 200 x 200 x 70: 66 tiles, one whole dealt round and a ragged rest."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import batched_ep_cases as X
import grouped_ep_cases as G
from qublas_amd import capi
from qublas_amd.desc import Qu, lower

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
FUSED, UNFUSED = G.FUSED, G.UNFUSED


@pytest.fixture(scope="module")
def ctx():
    with capi.Context() as c:
        yield c


def same(got, exp, what):
    for g, (a, b) in enumerate(zip(got, exp)):
        assert a.tobytes() == b.tobytes(), (what, g)


def check_forms(ctx, oracle, members, plain=True, want_in=None):
    """the whole comparison of one group; returns {flags: (fuses, launches)}"""
    exp = [m.expected(oracle) for m in members]
    dev = G.Device(ctx, oracle, members)
    forms = {}
    try:
        if plain:
            same(G.run_plain_loop(ctx, oracle, dev), exp, "plain loop")
        fusable = G.fusable(members)
        descs = [m.d for m in members]
        ch = members[0].chain
        for flags in (0, FUSED, UNFUSED):
            run = G.GroupedRun(ctx, dev, flags)
            try:
                same(run.run(), exp, ("grouped", flags))
                fused = fusable and flags == FUSED
                assert run.plan.fuses() == (1 if fused else 0), flags
                # classify_* equals what the created plan answers
                st, info = capi.classify_grouped_epx_status(descs, ch.ep, ch.tabs, ch.per_member, flags)
                assert st == capi.QG_OK and bytes(info.reason) == bytes(run.plan.info.reason) and list(info.packed_bytes) == list(run.plan.info.packed_bytes)
                assert run.plan.launches == capi.classify_grouped_epx_launches(descs, ch.ep, ch.tabs, ch.per_member, flags)
                for g in range(len(members)):
                    a, b = run.plan.member(g), capi.classify_grouped_epx_member(descs, ch.ep, g, ch.tabs, ch.per_member, flags)
                    assert bytes(a) == bytes(b), g
                if want_in is not None:
                    assert [run.plan.member(g).in_launch for g in range(len(members))] == want_in
                forms[flags] = (run.plan.fuses(), run.plan.launches)
            finally:
                run.close()
        return forms
    finally:
        dev.close()


CASES = ([(f, "1_scale_shared_bias") for f in sorted(X.FORMATS)] +
         [(f, "3_no_stage_narrow_sat") for f in ("e43_c1byte", "e88_3x3", "e88_x_e43_3x1_c16", "q78_centred_c16")] +
         [(f, "4_four_stages_1_2_4_8_bytes") for f in ("e43_c1byte", "e88_3x3", "q78_centred")] +
         [(f, "5_act_uniform") for f in ("e43_c1byte", "e88_3x3_c16")])


@pytest.mark.parametrize("fmt,chain", CASES, ids=lambda v: v)
def test_chain_forms_vs_oracle_and_plain_loop(ctx, oracle, fmt, chain):
    ch = G.Chain.named(fmt, chain)
    members = [G.fmt_member(oracle, fmt, s, ch, seed=100 + 7 * i, dist=i % 2) for i, s in enumerate(G.SHAPES + G.BIG)]
    for i, m in enumerate(members):                                            # every member has a distinct value in every scalar stage
        m.scal = [None if s is None else 5 * i - 23 + k for k, s in enumerate(m.scal)]
    forms = check_forms(ctx, oracle, members, want_in=[1] * len(members))
    fusable = G.fusable(members)
    if chain.startswith("1_"):
        assert fusable == (fmt == "e43_c1byte" or fmt.endswith("_c16")), fmt      # every limb geometry runs fused through the _c16 twins
    if chain.startswith(("4_", "5_")):
        assert not fusable
    assert forms == {0: (0, 2), FUSED: ((1, 1) if fusable else (0, 2)), UNFUSED: (0, 2)}


@pytest.mark.parametrize("fmt", ["e43_c1byte", "e88_3x3_c16"])
@pytest.mark.parametrize("chain,table", [("6_act_scalar_32bit", True), ("6_act_scalar_32bit", False), ("5_act_uniform", False)],
                         ids=["32bit_table", "32bit_call_wide", "64bit_call_wide"])
def test_approx_pass_arithmetic_and_scalar_source(ctx, oracle, fmt, chain, table):
    """k_approx_grp<int32_t / int64_t> with the scalar from the plan's table or call-wide: the branches that chain 5_act_uniform above
    (64-bit, table) leaves out.  Three members; oracle == plain loop == pass form, byte for byte"""
    ch = G.Chain.named(fmt, chain)
    members = [G.fmt_member(oracle, fmt, s, ch, seed=300 + 7 * i, dist=i % 2) for i, s in enumerate([(64, 64, 1), (3, 5, 7), (129, 130, 65)])]
    assert X.bits32(members[0].d, ch.ep, ch.tabs) == chain.endswith("_32bit") and not G.fusable(members)
    for i, m in enumerate(members):
        m.scal = [None if s is None else (5 * i - 23 + k if table else 11 - k) for k, s in enumerate(m.scal)]
    if table:
        assert check_forms(ctx, oracle, members, want_in=[1, 1, 1]) == {0: (0, 2), FUSED: (0, 2), UNFUSED: (0, 2)}
        return
    exp = [m.expected(oracle) for m in members]
    dev = G.Device(ctx, oracle, members)
    try:
        same(G.run_plain_loop(ctx, oracle, dev), exp, "plain loop")
        for flags in (0, UNFUSED):
            run = G.GroupedRun(ctx, dev, flags, per_member=[0] * len(ch.stages), e_scalar=[0 if s is None else s for s in members[0].scal])
            try:
                same(run.run(), exp, ("grouped", flags))
                assert (run.plan.fuses(), run.plan.launches) == (0, 2)
            finally:
                run.close()
    finally:
        dev.close()


def test_per_member_scalars_swap_and_reset(ctx, oracle):
    """every member has a distinct value; swapping two members' values swaps exactly their results; set_scalars after a first execute
    changes the next execute's D; a stage with scalar_per_member = 0 uses e_scalar[k]"""
    for fmt, flags in (("e43_c1byte", UNFUSED), ("e88_3x3_c16", FUSED), ("q78_centred_c16", FUSED)):
        ch = G.Chain(X.FORMATS[fmt][2], G.MIXED, G.D126)                       # scalar mul, tensor add, scalar sub
        members = [G.fmt_member(oracle, fmt, s, ch, seed=300 + 5 * i, dist=1) for i, s in enumerate(G.SHAPES)]
        for i, m in enumerate(members):                                         # distinct, non-trivial scales: 3, 4, 5, ... and offsets
            m.scal = [3 + i, None, 17 * i - 40]
        own = [m.scal for m in members]
        a, b = 1, 5                                                            # (3,5,7) and (65,33,100)
        swapped = list(own)
        swapped[a], swapped[b] = own[b], own[a]
        exp_own = [m.expected(oracle) for m in members]
        exp_swapped = [m.expected(oracle, s) for m, s in zip(members, swapped)]
        assert exp_own[a].tobytes() != exp_swapped[a].tobytes() and exp_own[b].tobytes() != exp_swapped[b].tobytes()
        dev = G.Device(ctx, oracle, members)
        try:
            same(G.run_plain_loop(ctx, oracle, dev, swapped), exp_swapped, "plain loop, swapped")
            run = G.GroupedRun(ctx, dev, flags)
            try:
                assert run.plan.fuses() == (1 if flags == FUSED else 0)
                same(run.run(), exp_own, (fmt, "own"))
                for k in (0, 2):
                    run.plan.set_scalars(k, [s[k] for s in swapped])
                got = run.run()                                                # the same plan, the same packed operands: only the tables changed
                same(got, exp_swapped, (fmt, "swapped"))
                assert [g for g in range(len(members)) if got[g].tobytes() != exp_own[g].tobytes()] == [a, b]
            finally:
                run.close()
            # stage 2 for all members from e_scalar[2], stage 0 still per member
            shared = [[s[0], None, -7] for s in own]
            run = G.GroupedRun(ctx, dev, flags, per_member=[1, 0, 0], e_scalar=[999, 0, -7])   # (e_scalar[0] is not read: stage 0 is per member)
            try:
                same(run.run(), [m.expected(oracle, s) for m, s in zip(members, shared)], (fmt, "shared stage 2"))
            finally:
                run.close()
        finally:
            dev.close()


@pytest.mark.parametrize("name", sorted(G.STRAGGLERS))
def test_straggler_kinds_carry_the_chain_with_their_own_scalar(ctx, oracle, name):
    a, b, c, kw, shape = G.STRAGGLERS[name]
    ch = G.Chain(X.E43, G.MIXED, G.D126)
    el = [G.fmt_member(oracle, "e43_c1byte", (3, 5, 7), ch, seed=800, dist=0), G.fmt_member(oracle, "e43_c1byte", (65, 33, 100), ch, seed=801, dist=1)]
    s1 = G.Member(oracle, a, b, c, shape, kw, ch, seed=810, dist=1)
    s2 = G.Member(oracle, a, b, c, (5, 3, shape[2]) if shape[2] > 1000 else (5, 9, shape[2]), kw, ch, seed=811, dist=1)
    members = [el[0], s1, s2, el[1]]                                           # (an eligible member first: the key is its own)
    for i, m in enumerate(members):
        m.scal = [2 + i, None, 11 - 9 * i]
    forms = check_forms(ctx, oracle, members, want_in=[1, 0, 0, 1])
    assert forms[FUSED][0] == 1 and forms[0][0] == 0


def test_leading_dimensions_with_poison_between_and_behind_the_members(ctx, oracle):
    for fmt, chain in (("e43_c1byte", "1_scale_shared_bias"), ("e88_3x3_tn_c16", "1_scale_shared_bias"), ("q78_centred", "4_four_stages_1_2_4_8_bytes")):
        ch = G.Chain.named(fmt, chain)
        ta = X.FORMATS[fmt][4]
        members = []
        for i, (M, N, K) in enumerate([(65, 33, 100), (0, 5, 7), (3, 130, 7), (64, 64, 65)]):
            ld = ((K if ta else M) + 3 + i, K + 5, M + 7 + i, M + 2 + i)
            members.append(G.fmt_member(oracle, fmt, (M, N, K), ch, seed=850 + i, dist=1 if i % 2 == 0 else 0, ld=ld))
        check_forms(ctx, oracle, members)                                      # (bytes outside D keep the poison: the buffers are compared whole)


@pytest.mark.parametrize("dists", [(1, 0), (0, 1), (1, 1)], ids=["small_then_full_range", "full_range_then_small", "all_small"])
def test_launch_wide_plane_mask_with_a_fused_chain(ctx, oracle, dists):
    """int<8,8> in three limb planes, fused: ONE plane mask for the launch decides which kernel of the pair stores D, so both partners
    carry the chain (all members small: the 2 x 2 partner; a full-range member anywhere: the 3 x 3 kernel)"""
    fmt = "e88_3x3_c16"
    ch = G.Chain.named(fmt, "1_scale_shared_bias")
    members = [G.fmt_member(oracle, fmt, s, ch, seed=500 + i, dist=dists[i]) for i, s in enumerate([(65, 33, 100), (3, 130, 7)])]
    forms = check_forms(ctx, oracle, members, plain=False)
    assert forms[FUSED] == (1, 1)
    assert len(set(np.concatenate([m.values(oracle) for m in members]).tolist())) > 100


@pytest.mark.parametrize("fmt", ["e43_c1byte", "e88_3x3_c16"])
def test_more_workgroups_than_cus(ctx, oracle, fmt):
    ch = G.Chain.named(fmt, "1_scale_shared_bias")
    rng = np.random.RandomState(20261019)
    shapes = [(int(rng.randint(1, 65)), int(rng.randint(1, 65)), int(rng.randint(1, 200))) for _ in range(300)]
    members = [G.fmt_member(oracle, fmt, s, ch, seed=700 + i, dist=i % 2) for i, s in enumerate(shapes)]
    exp = [m.expected(oracle) for m in members]
    dev = G.Device(ctx, oracle, members)
    try:
        for flags, form in ((FUSED, (1, 1)), (UNFUSED, (0, 2))):
            run = G.GroupedRun(ctx, dev, flags)
            try:
                assert (run.plan.fuses(), run.plan.launches) == form
                same(run.run(), exp, (fmt, flags))
            finally:
                run.close()
    finally:
        dev.close()


def test_packed_e_bytes_answers_for_the_group(ctx):
    fmt = "e88_3x3"
    ea, eb, ec, kw, ta, _ = X.FORMATS[fmt]
    ch = G.Chain.named(fmt, "4_four_stages_1_2_4_8_bytes")
    shapes = [(65, 33, 100), (3, 5, 7), (129, 130, 65)]
    tree = lower(X.E88, X.E88, ec, 33, 17, 40)                                  # default tags: the tree class, a straggler of the same C
    descs = [lower(ea, eb, ec, M, N, K, **kw) for M, N, K in shapes] + [tree]
    plan = capi.GroupedPlan(ctx, descs, ep=ch.ep, approx=ch.tabs, per_member=ch.per_member)
    try:
        assert [plan.member(g).in_launch for g in range(4)] == [1, 1, 1, 0]
        tiles = 2 + 1 + 9
        one = capi.Plan(ctx, tree, epilogue=ch.ep, approx=ch.tabs)
        for k, ebytes in enumerate((1, 2, 4, 8)):
            launch = tiles * 4096 * ebytes
            assert plan.packed_e_bytes(k) == (launch + 255) // 256 * 256 + one.packed_e_bytes(k), k
        assert plan.packed_e_bytes(4) == 0 and plan.packed_e_bytes(-1) == 0
        one.close()
    finally:
        plan.close()


def test_entry_points_refuse_each_other(ctx):
    d, ep, tabs, stages, ec, dq, shared = X.lowered("e43_c1byte", (64, 64, 64), "1_scale_shared_bias")
    gep = capi.GroupedPlan(ctx, [d, d], ep=ep, per_member=[1, 0])
    gp, bp, bep, pp, pep = capi.GroupedPlan(ctx, [d, d]), capi.BatchedPlan(ctx, d, 2), capi.BatchedPlan(ctx, d, 2, ep=ep, shared=shared), capi.Plan(ctx, d), capi.Plan(ctx, d, epilogue=ep)
    buf = ctx.alloc(1 << 18)
    L, v = capi.lib(), C.c_void_p
    args = capi.Plan.ep_args(packed=[0, buf + (1 << 17)], scalars=[3, 0])
    ptrs = (v * 2)(v(buf), v(buf))
    vals = (C.c_int64 * 2)(3, 4)
    ms = C.c_float()
    EINVAL = capi.QG_EINVAL
    try:
        # qgemul_execute_grouped refuses a grouped plan with a chain, as qgemul_execute refuses a plain plan with one
        assert L.qgemul_execute_grouped(gep.h, v(buf), v(buf), v(buf)) == EINVAL
        assert L.qgemul_time_execute_grouped(gep.h, v(buf), v(buf), v(buf), 0, 1, C.byref(ms)) == EINVAL
        # the plain and the batched entry points refuse the new plan
        assert L.qgemul_execute(gep.h, v(buf), v(buf), v(buf)) == EINVAL
        assert L.qgemul_execute_ep(gep.h, v(buf), v(buf), v(buf), C.byref(args)) == EINVAL
        assert L.qgemul_pack(gep.h, 0, v(buf), 0, v(buf)) == EINVAL
        assert L.qgemul_pack_e(gep.h, 1, v(buf), 0, v(buf)) == EINVAL
        assert L.qgemul_pack_c(gep.h, v(buf), 0, v(buf)) == EINVAL
        assert L.qgemul_apply_epilogue(gep.h, v(buf), v(buf), C.byref(args)) == EINVAL
        assert L.qgemul_unpack_c(gep.h, v(buf), v(buf), 0) == EINVAL
        assert L.qgemul_time_execute_ep(gep.h, v(buf), v(buf), v(buf), C.byref(args), 0, 1, C.byref(ms)) == EINVAL
        assert L.qgemul_export_bitstream(gep.h, v(buf), 0, 0, 0, v(buf)) == EINVAL
        assert L.qgemul_execute_batched(gep.h, v(buf), v(buf), v(buf)) == EINVAL
        assert L.qgemul_execute_batched_ep(gep.h, v(buf), v(buf), v(buf), C.byref(args)) == EINVAL
        assert L.qgemul_pack_e_batched(gep.h, 1, v(buf), 0, 4096, v(buf)) == EINVAL
        assert L.qgemul_unpack_c_batched(gep.h, v(buf), v(buf), 0, 4096) == EINVAL
        assert L.qgemul_plan_batched_launches(gep.h) == EINVAL
        # the _grouped_ep entries refuse a grouped plan without a chain, plain plans and batched plans
        for h in (gp.h, pp.h, pep.h, bp.h, bep.h):
            assert L.qgemul_execute_grouped_ep(h, v(buf), v(buf), v(buf), C.byref(args)) == EINVAL
            assert L.qgemul_pack_e_grouped(h, 1, ptrs, None, v(buf)) == EINVAL
            assert L.qgemul_grouped_set_scalars(h, 0, vals) == EINVAL
            assert L.qgemul_time_execute_grouped_ep(h, v(buf), v(buf), v(buf), C.byref(args), 0, 1, C.byref(ms)) == EINVAL
        # executing while a per-member stage's table was never set
        assert L.qgemul_execute_grouped_ep(gep.h, v(buf), v(buf), v(buf), C.byref(args)) == EINVAL
        # a stage that is not a per-member scalar stage; a missing table; a scalar stage at qgemul_pack_e_grouped; a missing operand
        assert L.qgemul_grouped_set_scalars(gep.h, 1, vals) == EINVAL
        assert L.qgemul_grouped_set_scalars(gep.h, 2, vals) == EINVAL
        assert L.qgemul_grouped_set_scalars(gep.h, 0, None) == EINVAL
        assert L.qgemul_pack_e_grouped(gep.h, 0, ptrs, None, v(buf)) == EINVAL
        bad_ld = (C.c_int64 * 2)(64, 63)
        assert L.qgemul_pack_e_grouped(gep.h, 1, ptrs, bad_ld, v(buf)) == EINVAL
        ptrs[1] = None
        assert L.qgemul_pack_e_grouped(gep.h, 1, ptrs, None, v(buf)) == EINVAL
        assert L.qgemul_grouped_set_scalars(gep.h, 0, vals) == capi.QG_OK
        none = capi.Plan.ep_args(packed=[0, 0], scalars=[3, 0])
        assert L.qgemul_execute_grouped_ep(gep.h, v(buf), v(buf), v(buf), C.byref(none)) == EINVAL
        # scalar_per_member on a tensor stage at plan creation
        h = v()
        assert L.qgemul_plan_create_grouped_epx(ctx.h, capi._desc_array([d, d]), 2, C.byref(ep), None, C.byref(capi.grouped_ep([0, 1])), 0, C.byref(h)) == EINVAL
        # what serves the new plan: info, launches, member (D), the timed execute
        info = capi.qgemul_info()
        assert L.qgemul_plan_info(gep.h, C.byref(info)) == capi.QG_OK and b"grouped chain pass: 2 members in one launch" in bytes(info.reason)
        assert (gep.fuses(), gep.launches) == (0, 2)
        rec = gep.member(1)
        assert (rec.in_launch, rec.off[2], rec.bytes[2]) == (1, 4096, 4096) and gep.packed_e_bytes(1) == 2 * 4096 * 4
        assert gep.time_execute_ep(buf, buf + 32768, buf + 65536, args, 1, 2) > 0
    finally:
        ctx.free(buf)
        for p in (gep, gp, bp, bep, pp, pep):
            p.close()


def test_one_shot_replans_over_list_chain_and_pattern_not_over_values(oracle):
    fmt = "q78_centred_c16"
    ch = G.Chain(X.FORMATS[fmt][2], G.MIXED, G.D126)
    ch2 = G.Chain.named(fmt, "1_scale_shared_bias")

    def group(chain, k_last):
        ms = [G.fmt_member(oracle, fmt, s, chain, seed=870 + i, dist=1 if i == 0 else 0) for i, s in enumerate([(65, 33, 100), (3, 5, 7), (33, 17, k_last)])]
        for i, m in enumerate(ms):
            m.scal = [(3 + i if s is not None else None) for s in m.scal]
        return ms

    def run(members, per_member=None, scal=None, flags=0):
        chain = members[0].chain
        pm = chain.per_member if per_member is None else per_member
        scal = [m.scal for m in members] if scal is None else scal
        Ds = [np.full(m.ext[2], 0x5a5a5a5a, dtype=oracle.host_dtype(chain.dq)) for m in members]
        E, S = [], []
        for k, st in enumerate(chain.stages):
            if G.is_tensor(st):
                E.append([m.E[k] for m in members]); S.append(None)
            elif pm[k]:
                E.append(None); S.append([s[k] for s in scal])
            else:
                E.append(np.asarray([scal[0][k]], dtype=oracle.host_dtype(st.e))); S.append(None)
        capi.run_grouped_epx([m.d for m in members], chain.ep, chain.tabs, pm, Ds, [m.A for m in members], [m.B for m in members], E, S, flags=flags)
        want = [m.values(oracle, [s[k] if pm[k] else scal[0][k] for k in range(len(s))]) for m, s in zip(members, scal)]
        for g, (d, w) in enumerate(zip(Ds, want)):
            assert d.tobytes() == w.tobytes(), g

    try:
        g1, g2, g3 = group(ch, 64), group(ch, 65), group(ch2, 64)
        run(g1)
        run(g1)                                                                # the cached plan
        run(g1, scal=[[9 - i, None, 5 * i] for i in range(3)])                 # changed values: the same plan, new tables
        run(g2)                                                                # the list changed
        run(g3)                                                                # the chain changed
        run(g1, per_member=[1, 0, 0])                                          # the pattern changed: stage 2 from one element for all
        run(g1, flags=FUSED)
        run(g1)
        m = g1[0]
        c = np.zeros(m.ext[2], dtype=oracle.host_dtype(m.ec))
        capi.run(m.d, c, m.A, m.B)                                             # a plain call takes the cache, the grouped call takes it back
        run(g1)
        Ds = [np.zeros(m.ext[2], dtype=oracle.host_dtype(ch.dq)) for m in g1]
        assert capi.run_grouped_epx_status([m.d for m in g1], ch.ep, ch.tabs, ch.per_member, Ds, [m.A for m in g1], [m.B for m in g1], [None, [m.E[1] for m in g1], None],
                                           [[1, 2, 3], None, [4, 5, 6]], flags=capi.OPT_ALL_DEVICES) == capi.QG_EUNSUPPORTED
    finally:
        capi.run_release()


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_grouped_chain_program(tmp_path, oracle):
    """tests/binding/amd_header_grouped_ep_run.cpp: QgemulGrouped<tags..., QgemulResult<CT>>(std::tie(D0, D1, D2), std::tie(A...), std::tie(B...),
    ThenMul(PerMember(s0, s1, s2)), ThenAdd(std::tie(Bias0, Bias1, Bias2)), ThenSub(offset)) on tensors of three dim<> through include/QuBLAS_amd.h"""
    from qublas_amd.desc import Ew, RND, SAT, TRN, Tags
    exe = tmp_path / "amd_header_grouped_ep_run"
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++23", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "binding", "amd_header_grouped_ep_run.cpp"), "-o", str(exe), "-L" + lib, "-lqugemm", "-Wl,-rpath," + lib])
    r = json.loads(subprocess.check_output([str(exe)], text=True).strip().splitlines()[-1])
    assert r.get("name") == "per_member_scale_tied_bias", r
    e88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
    ct, t1, dt = Qu(7, 8), Qu(20, 8), Qu(12, 6, True, RND.CONV, SAT.TCPL)
    stages = [Ew("mul", X.S34, Tags(20, 8), scalar=True, into=t1), Ew("add", X.B106, into=t1), Ew("sub", X.S34, scalar=True)]
    gen = lambda n, mul, add, mod, off: (((np.arange(n, dtype=np.uint64) * np.uint64(mul) + np.uint64(add)) % np.uint64(mod)).astype(np.int64) - off)
    layers = [((65, 33, 40), (2654435761, 0), (40503, 7), (97, 0)), ((3, 130, 100), (2246822519, 3), (3266489917, 11), (131, 5)), ((64, 64, 7), (668265263, 5), (374761393, 13), (193, 9))]
    seen = set()
    for g, ((M, N, K), fa, fb, fe) in enumerate(layers):
        d = lower(e88, e88, ct, M, N, K, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
        A, B = gen(M * K, *fa, 128, 64).astype(np.int32), gen(K * N, *fb, 128, 64).astype(np.int32)
        bias = gen(M * N, *fe, 512, 256)
        Cx = oracle.gemm(d, A, B, ct).astype(np.int64)
        exp = X.expected(oracle, ct, stages, dt, Cx, [np.asarray([r["scales"][g]], dtype=np.int64), bias, np.asarray([r["offset"]], dtype=np.int64)])
        assert r[f"D{g}"] == np.asarray(exp).astype(np.int64).tolist(), g
        seen |= set(r[f"D{g}"])
    assert len(seen) > 20
