"""Element-wise chains on batched plans: what the planner decides, pure host code (no GPU).  Which of the three forms a chain takes
(fused into the block-diagonal launch / one block-diagonal pass behind it / member by member) and how many launches that is, for
every format row x chain x placement flag; the sizes the plan reports; that the status is the member descriptor's own
qgemul_classify_epx status; every QG_EINVAL that needs no device; overflow of the stacked sizes."""
import ctypes as C

import pytest

import batched_ep_cases as X
from qublas_amd import capi
from qublas_amd.desc import Approx, Ew, Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, lower, lower_epilogue, lower_epilogue_x

FUSED, UNFUSED = capi.OPT_FUSED_EPILOGUE, capi.OPT_UNFUSED_EPILOGUE
CHAINS = sorted(X.chains(X.E43))


@pytest.mark.parametrize("chain", CHAINS)
@pytest.mark.parametrize("fmt", sorted(X.FORMATS))
def test_form_and_launch_count(fmt, chain):
    for shape in X.SHAPES:
        d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, shape, chain)
        fusable = X.bits32(d, ep, tabs) and not X.has_approx(stages)
        for batch in X.BATCHES:
            assert list(capi.classify_batched_epx_status(d, batch, ep, tabs, shared)[1].limbs) == X.FORMATS[fmt][5]
            for flags in (0, FUSED, UNFUSED, FUSED | UNFUSED):
                st, info = capi.classify_batched_epx_status(d, batch, ep, tabs, shared, flags)
                assert st == capi.QG_OK, info.reason
                fused = X.fused_expected(fusable, flags)                 # (QG_OPT_UNFUSED_EPILOGUE always wins)
                assert capi.classify_batched_epx_launches(d, batch, ep, tabs, shared, flags) == (1 if fused else 2), (fmt, chain, shape, batch, flags)
                assert (b"chain fused into one block-diagonal launch" if fused else b"one chain pass over the stack") in bytes(info.reason), info.reason


def test_which_chains_can_fuse():
    """chain 1 is a 32-bit chain wherever C has at most 32 storage bits; chains 2 and 4 never are; an APPROX stage never fuses"""
    for fmt in X.FORMATS:
        ec = X.FORMATS[fmt][2]
        for chain in CHAINS:
            d, ep, tabs, stages, _, _, _ = X.lowered(fmt, (65, 33, 100), chain)
            b32 = X.bits32(d, ep, tabs)
            if chain.startswith("1_"):
                assert b32 == (ec.storage_bits <= 16), (fmt, ec)
            if chain.startswith(("2_", "4_")):
                assert not b32
    assert sum(1 for f in X.FORMATS if X.FORMATS[f][2].storage_bits <= 16) == 5      # 1 x 1 and the four limb twins: every fused geometry


def test_sizes_describe_d_and_the_stacked_operands():
    for fmt in ("e43_c1byte", "e88_3x3", "q78_centred_c16"):
        for chain in CHAINS:
            d, ep, tabs, stages, ec, dq, shared = X.lowered(fmt, (65, 33, 100), chain)
            _, one = capi.classify_epx(d, ep, tabs)
            tiles = 2 * 1 * 64 * 64
            for batch in (1, 9):
                st, info = capi.classify_batched_epx_status(d, batch, ep, tabs, shared)
                assert st == capi.QG_OK
                assert info.host_elem_bytes[2] == one.host_elem_bytes[2] == dq.host_bytes
                dbytes = next(b for b in (1, 2, 4, 8) if 8 * b >= dq.storage_bits)
                assert info.packed_bytes[2] == batch * tiles * dbytes
                assert info.ops == batch * one.ops


FALLBACKS = {
    # name -> (operand element, C element, lowering keywords, GEMM launches per member)
    "tree_default_tags": (X.E88, X.E88, {}, 1),
    "ring_int16": (Qu(15, 0, True, TRN.TCPL, WRP.TCPL), Qu(15, 0, True, TRN.TCPL, WRP.TCPL), {}, 1),
    "raw_pass_left_shift": (Qu(10, -3), Qu(24, 9), dict(mul_args=Tags(21, -6), add_args=[Qu(28, -6)]), 2),
}


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_fallback_counts(name):
    e, ec, kw, gemm_launches = FALLBACKS[name]
    d = lower(e, e, ec, 33, 17, 40, **kw)
    stages = [Ew("mul", X.S34, scalar=True, into=ec), Ew("add", X.B106, into=ec), Ew("sub", X.B106)]
    ep, tabs = lower_epilogue_x(ec, stages, ec)
    for flags in (0, FUSED, UNFUSED):
        st, info = capi.classify_batched_epx_status(d, 3, ep, tabs, [0, 1, 0], flags)
        assert st == capi.QG_OK and b"member by member" in bytes(info.reason), info.reason
        assert capi.classify_batched_epx_launches(d, 3, ep, tabs, [0, 1, 0], flags) == 3 * (gemm_launches + 1)     # (none of these kernels fuses a chain)
    # a member large enough for the two-group kernels has no block-diagonal form either
    big = lower(X.E43, X.E43, Qu(4, 3), 4096, 4096, 64, mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
    ep1, t1 = lower_epilogue_x(Qu(4, 3), X.chains(Qu(4, 3))["1_scale_shared_bias"][0], Qu(4, 3))
    assert capi.classify_batched_epx_launches(big, 2, ep1, t1, [0, 1]) == 2 * 2
    assert capi.classify_batched_epx_launches(big, 2, ep1, t1, [0, 1], FUSED) == 2 * 1


def test_struct_mirror_is_the_headers_struct():
    """uint8_t e_shared[QG_MAX_EW]; uint8_t reserved[4];  (qgemul_packed_e_bytes takes a plan, which takes a device: tests/test_gpu_batched_ep.py)"""
    assert C.sizeof(capi.qgemul_batched_ep) == 8 and capi.qgemul_batched_ep.e_shared.offset == 0 and capi.qgemul_batched_ep.reserved.offset == 4
    assert list(capi.batched_ep([0, 1, 1]).e_shared) == [0, 1, 1, 0]


def status_cases():
    c8, wide = Qu(4, 3), Qu(24, 8)
    ok = lower(X.E43, X.E43, c8, 65, 33, 100, mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
    cplx_e = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
    cplx = lower(cplx_e, cplx_e, cplx_e, 33, 17, 40, mul_args=TFComplexMul())
    out = []
    for name, (stages, dq, _) in X.chains(c8).items():
        out.append((name, ok, c8, stages, dq))
    out.append(("complex_member", cplx, c8, [Ew("add", X.B106)], c8))
    out.append(("tcpl_sat_d", ok, c8, [Ew("add", X.B106)], Qu(2, 2, True, TRN.TCPL, WRP.TCPL_SAT)))
    out.append(("operand_wider_than_62", ok, c8, [Ew("mul", Qu(40, 30))], Qu(20, 8)))
    return out


@pytest.mark.parametrize("case", status_cases(), ids=lambda c: c[0])
def test_status_is_the_member_descriptors_own(case):
    name, d, c, stages, dq = case
    ep, tabs = lower_epilogue_x(c, stages, dq)
    want, winfo = capi.classify_epx(d, ep, tabs)
    for batch in (1, 9):
        got, info = capi.classify_batched_epx_status(d, batch, ep, tabs, [0] * len(stages))
        assert got == want, (name, info.reason, winfo.reason)
        n = capi.classify_batched_epx_launches(d, batch, ep, tabs, [0] * len(stages))
        assert (n > 0) if want == capi.QG_OK else (n == want)
    if name in ("complex_member", "tcpl_sat_d", "operand_wider_than_62"):
        assert want != capi.QG_OK


def test_malformed_chains_keep_their_status():
    d, ep, tabs, stages, ec, dq, shared = X.lowered("e43_c1byte", (65, 33, 100), "5_act_uniform")
    # a missing table, a surplus table, too many stages, an unknown op
    for bad_tabs in ([None] * 4, [tabs[2], None, tabs[2], None]):
        want = capi.classify_epx(d, ep, bad_tabs)[0]
        assert want == capi.QG_EINVAL == capi.classify_batched_epx_status(d, 2, ep, bad_tabs, shared)[0]
    ep.n_stages = 5
    assert capi.classify_batched_epx_status(d, 2, ep, tabs, shared)[0] == capi.classify_epx(d, ep, tabs)[0] != capi.QG_OK
    ep.n_stages = 3
    ep.stage[0].op = 9
    assert capi.classify_batched_epx_status(d, 2, ep, tabs, shared)[0] == capi.classify_epx(d, ep, tabs)[0] != capi.QG_OK


def test_einval_without_a_device():
    L = capi.lib()
    d, ep, tabs, stages, ec, dq, shared = X.lowered("e43_c1byte", (65, 33, 100), "1_scale_shared_bias")
    info = capi.qgemul_info()
    for batch in (0, -3):
        assert capi.classify_batched_epx_status(d, batch, ep, tabs, shared)[0] == capi.QG_EINVAL
        assert capi.classify_batched_epx_launches(d, batch, ep, tabs, shared) == capi.QG_EINVAL
    assert L.qgemul_classify_batched_epx(None, 2, C.byref(ep), None, None, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_batched_epx(C.byref(d), 2, None, None, None, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_batched_epx(C.byref(d), 2, C.byref(ep), None, None, 0, None) == capi.QG_EINVAL
    assert L.qgemul_classify_batched_epx_launches(C.byref(d), 2, None, None, None, 0) == capi.QG_EINVAL
    plan = C.c_void_p()
    assert L.qgemul_plan_create_batched_epx(None, C.byref(d), 2, C.byref(ep), None, None, 0, C.byref(plan)) == capi.QG_EINVAL
    # ax == NULL means no APPROX stage, bep == NULL that no stage is shared: both are valid
    assert L.qgemul_classify_batched_epx(C.byref(d), 2, C.byref(ep), None, None, 0, C.byref(info)) == capi.QG_OK
    # null plans
    v = C.c_void_p
    ms = C.c_float()
    assert L.qgemul_pack_e_batched(None, 0, v(16), 0, 0, v(16)) == capi.QG_EINVAL
    assert L.qgemul_execute_batched_ep(None, v(16), v(16), v(16), None) == capi.QG_EINVAL
    assert L.qgemul_time_execute_batched_ep(None, v(16), v(16), v(16), None, 0, 1, C.byref(ms)) == capi.QG_EINVAL
    # the one-shot entry validates before it touches a device: null pointers, batch, strides below the extents, a tensor stage
    # without a stride list, the sharded flag
    import numpy as np
    z = np.zeros(8, dtype=np.int32)
    extA, extB, extD = X.extents(d)
    E, sE = [z, z], [0, 0, 0, 0]
    run = lambda batch=2, sD=extD, sA=extA, sB=extB, sE=sE, **kw: capi.run_batched_epx_status(d, batch, ep, tabs, z, z, z, E, sD, sA, sB, sE, **kw)
    assert run(batch=0) == capi.QG_EINVAL
    assert run(sD=extD - 1) == run(sA=extA - 1) == run(sB=0) == capi.QG_EINVAL
    assert run(sE=[0, extD - 1, 0, 0]) == capi.QG_EINVAL                     # a per-member stride below the operand's extent
    assert run(flags=capi.OPT_ALL_DEVICES) == capi.QG_EUNSUPPORTED
    o = capi.qgemul_opts(0, 0, 0, -1, 0)
    ptrs = (C.c_void_p * 4)(z.ctypes.data, z.ctypes.data, None, None)
    call = lambda D, E, sE: L.qgemul_run_batched_epx(C.byref(d), 2, C.byref(ep), None, D, z.ctypes.data_as(v), z.ctypes.data_as(v), E, extD, extA, extB, sE, C.byref(o))
    assert call(None, ptrs, (C.c_int64 * 4)(0, 0, 0, 0)) == capi.QG_EINVAL
    assert call(z.ctypes.data_as(v), None, (C.c_int64 * 4)(0, 0, 0, 0)) == capi.QG_EINVAL
    assert call(z.ctypes.data_as(v), ptrs, None) == capi.QG_EINVAL


def test_overflow_of_the_stacked_sizes():
    d, ep, tabs, stages, ec, dq, shared = X.lowered("e43_c1byte", (64, 64, 64), "2_member_sub_shared_mul_wide")
    assert capi.classify_batched_epx_status(d, 1 << 20, ep, tabs, shared)[0] == capi.QG_OK
    st, info = capi.classify_batched_epx_status(d, 1 << 31, ep, tabs, shared)          # more than 2^31 - 1 tiles
    assert st == capi.QG_EINVAL and info.supported == 0, info.reason
    st, info = capi.classify_batched_epx_status(d, (1 << 62) + 5, ep, tabs, shared)    # the products wrap
    assert st == capi.QG_EINVAL
    # member by member: D and the stacked per-member operands are counted too
    e = X.E88
    t = lower(e, e, e, 33, 17, 40)
    ept, tt = lower_epilogue_x(e, [Ew("add", Qu(30, 10))], Qu(30, 12))
    assert capi.classify_batched_epx_status(t, 1 << 20, ept, tt, [0])[0] == capi.QG_OK
    assert capi.classify_batched_epx_status(t, 1 << 50, ept, tt, [0])[0] == capi.QG_EINVAL
    assert capi.classify_batched_epx_launches(t, 1 << 50, ept, tt, [0]) == capi.QG_EINVAL
