"""The planner of the grouped Qgemul through the built library, without a GPU (the qgemul_classify_grouped* functions are pure host
code): which members share the one launch, the launch counts, the packed layout and the refusals."""
import ctypes as C

import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, lower

E43, E88, U8, Q78, W16 = Qu(4, 3), Qu(8, 8), Qu(8, 0, False), Qu(7, 8), Qu(16, 3)
L43 = dict(mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
L88 = dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
LU8 = dict(mul_args=Tags(16, 0, False), add_args=[Qu(28, 0, False)])
LQ78 = dict(mul_args=Tags(15, 16), add_args=[Qu(28, 16)])
SHAPES = [(1, 1, 1), (3, 5, 7), (64, 64, 64), (65, 33, 100), (129, 130, 65), (64, 64, 300), (130, 10, 700)]
C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
I16 = Qu(15, 0, True, TRN.TCPL, WRP.TCPL)
# name -> (operand element, C element, lowering keywords, launches per member)   (FALLBACKS of tests/test_gpu_batched.py)
FALLBACKS = {
    "tree_default_tags": (E88, E88, {}, 1),
    "complex_tf": (C5, C5, dict(mul_args=TFComplexMul()), 1),
    "ring_int16": (I16, I16, {}, 1),
    "raw_pass_left_shift": (Qu(10, -3), Qu(24, 9), dict(mul_args=Tags(21, -6), add_args=[Qu(28, -6)]), 2),
}
# name -> (elements, C, keywords, trailer bytes per operand, centred)
ELIGIBLE = {
    "e43": (E43, Qu(4, 3), L43, 0, False),
    "e88": (E88, Qu(24, 8), L88, 256, False),
    "u8_centred": (U8, Qu(26, 0, False), LU8, 0, True),
    "q78_centred": (Q78, Qu(20, 8), LQ78, 256, True),
}


def group(name, shapes=SHAPES):
    e, ec, kw, _, _ = ELIGIBLE[name]
    return [lower(e, e, ec, M, N, K, **kw) for M, N, K in shapes]


def members(descs):
    return [capi.classify_grouped_member(descs, g) for g in range(len(descs))]


def up(x, m):
    return (x + m - 1) // m * m


def test_struct_mirror_matches_the_library():
    assert capi.sizeof(12) == C.sizeof(capi.qgemul_grouped_member) > 0
    assert capi.SIZEOF_MIRRORS[12] is capi.qgemul_grouped_member


@pytest.mark.parametrize("name", sorted(ELIGIBLE))
def test_all_eligible_groups_are_one_launch(name):
    descs = group(name)
    st, info = capi.classify_grouped_status(descs)
    assert st == capi.QG_OK and b"7 members in one launch" in bytes(info.reason) and b"0 run alone" in bytes(info.reason), info.reason
    assert capi.classify_grouped_launches(descs) == 1
    recs = members(descs)
    assert all(r.in_launch == 1 and r.launches == 0 for r in recs)
    bk = 128 if list(info.limbs) == [1, 1] else 64
    for d, r in zip(descs, recs):
        assert (r.tiles_m, r.tiles_n, r.k_tiles) == (up(d.M, 64) // 64, up(d.N, 64) // 64, up(d.K, bk) // bk)
    assert info.ops == sum(2.0 * d.M * d.N * d.K for d in descs)


@pytest.mark.parametrize("name", sorted(ELIGIBLE))
def test_packed_bytes_are_members_plus_one_trailer_plus_one_row_sum_array(name):
    _, _, _, trailer, centred = ELIGIBLE[name]
    descs = group(name)
    info = capi.classify_grouped_status(descs)[1]
    recs = members(descs)
    for w, rows in ((0, sum(up(d.M, 64) for d in descs)), (1, sum(up(d.N, 64) for d in descs))):
        want = sum(r.bytes[w] for r in recs) + trailer
        if centred:
            want = up(want, 256) + rows * 8
        assert info.packed_bytes[w] == want, (name, w)
        limbs = info.limbs[w]
        bk = 128 if list(info.limbs) == [1, 1] else 64
        for d, r in zip(descs, recs):
            assert r.bytes[w] == limbs * up(d.M if w == 0 else d.N, 64) * up(d.K, bk)
    assert info.packed_bytes[2] == sum(r.bytes[2] for r in recs)


@pytest.mark.parametrize("name", sorted(ELIGIBLE))
def test_member_offsets_neither_overlap_nor_leave_the_1024_byte_alignment(name):
    descs = group(name, SHAPES + SHAPES[::-1])
    recs = members(descs)
    for w in range(3):
        end = 0
        for r in recs:
            assert r.off[w] % 1024 == 0 and r.off[w] == end, (name, w)
            end = r.off[w] + r.bytes[w]


@pytest.mark.parametrize("name", sorted(FALLBACKS))
def test_straggler_kinds_run_alone_behind_the_launch(name):
    e, ec, kw, per_member = FALLBACKS[name]
    el = group("e43", [(3, 5, 7), (65, 33, 100)])
    s = [lower(e, e, ec, 33, 17, 40, **kw), lower(e, e, ec, 5, 9, 40, **kw)]
    descs = [s[0], el[0], s[1], el[1]]
    st, info = capi.classify_grouped_status(descs)
    assert st == capi.QG_OK and b"2 members in one launch" in bytes(info.reason) and b"2 run alone" in bytes(info.reason), info.reason
    assert capi.classify_grouped_launches(descs) == 1 + 2 * per_member
    recs = members(descs)
    assert [r.in_launch for r in recs] == [0, 1, 0, 1] and [r.launches for r in recs] == [per_member, 0, per_member, 0]
    for w in range(3):
        # the launch's part first (no trailer, no row sums for int<4,3>), the stragglers behind it at 256-byte-aligned offsets in
        # the layout of their own plain plans
        end = recs[1].bytes[w] + recs[3].bytes[w]
        assert recs[1].off[w] == 0 and recs[3].off[w] == recs[1].bytes[w]
        for g in (0, 2):
            plain = capi.classify(descs[g])
            assert recs[g].off[w] == up(end, 256) and recs[g].bytes[w] == plain.packed_bytes[w]
            end = recs[g].off[w] + recs[g].bytes[w]
        assert info.packed_bytes[w] == end


def test_a_second_key_runs_alone():
    """the key is that of the first eligible member in list order"""
    e88, e43 = group("e88", [(65, 33, 100), (3, 5, 7)]), group("e43", [(3, 5, 7), (65, 33, 100)])
    assert [r.in_launch for r in members(e88 + e43)] == [1, 1, 0, 0] and capi.classify_grouped_launches(e88 + e43) == 3
    assert [r.in_launch for r in members(e43 + e88)] == [1, 1, 0, 0]
    assert [r.in_launch for r in members([e43[0], e88[0], e43[1], e88[1]])] == [1, 0, 1, 0]
    # a different C container or a different conversion into C is a different key as well
    other_c = lower(E43, E43, W16, 3, 5, 7, **L43)
    assert [r.in_launch for r in members([e43[0], other_c, e43[1]])] == [1, 0, 1]
    # a straggler first: the key is still the first ELIGIBLE member's
    tree = lower(E88, E88, E88, 33, 17, 40)
    assert [r.in_launch for r in members([tree] + e43)] == [0, 1, 1]
    # no eligible member at all: every member alone
    assert [r.in_launch for r in members([tree, tree])] == [0, 0] and capi.classify_grouped_launches([tree, tree]) == 2


def test_a_member_large_enough_for_the_two_group_kernel_runs_alone():
    e43 = group("e43", [(3, 5, 7), (65, 33, 100)])
    big = lower(E43, E43, Qu(4, 3), 4096, 4096, 64, **L43)
    assert capi.classify(big).packed_bytes[0] == 4096 * 128      # (256 x 256 tiles on 128-byte k-tiles: the plain plan's own layout)
    descs = [e43[0], big, e43[1]]
    recs = members(descs)
    assert [r.in_launch for r in recs] == [1, 0, 1] and capi.classify_grouped_launches(descs) == 2
    assert recs[1].bytes[0] == capi.classify(big).packed_bytes[0]
    big33 = lower(E88, E88, Qu(24, 8), 2048, 2048, 64, **L88)          # 3 x 3 limbs with a tile per CU: the two-group limb kernel
    e88 = group("e88", [(3, 5, 7)])
    assert [r.in_launch for r in members(e88 + [big33])] == [1, 0]


def test_the_exact_range_of_the_int32_accumulators_decides_eligibility():
    """min(LA, LB) * K = 2^17 leaves the one-launch kernels' exact range: such a member is a straggler, 2^17 - 1 stays in the launch"""
    kw = dict(mul_args=Tags(9, 6), add_args=[Qu(27, 6)])
    mk = lambda K: lower(E43, E43, Qu(13, 6), 2, 3, K, **kw)
    recs = members([mk(64), mk(131071), mk(131072)])
    assert [r.in_launch for r in recs] == [1, 1, 0] and recs[1].k_tiles == 1024
    kw2 = dict(mul_args=Tags(15, 14), add_args=[Qu(32, 14)])
    mk2 = lambda K: lower(Qu(7, 7), Qu(7, 7), Qu(20, 7), 2, 3, K, **kw2)
    recs = members([mk2(64), mk2(65535), mk2(65536)])
    assert [r.in_launch for r in recs] == [1, 1, 0] and recs[1].k_tiles == 1024


def test_identical_descriptors_report_the_batched_plans_bytes():
    for name in sorted(ELIGIBLE):
        d = group(name, [(65, 33, 100)])[0]
        for batch in (1, 2, 9):
            g, b = capi.classify_grouped_status([d] * batch)[1], capi.classify_batched_status(d, batch)[1]
            assert list(g.packed_bytes) == list(b.packed_bytes), (name, batch)
            assert capi.classify_grouped_launches([d] * batch) == capi.classify_batched_launches(d, batch) == 1


def test_empty_members_take_no_tile():
    e, ec, kw, _, _ = ELIGIBLE["e43"]
    descs = [lower(e, e, ec, 0, 5, 7, **kw), lower(e, e, ec, 65, 33, 100, **kw), lower(e, e, ec, 9, 0, 64, **kw)]
    recs = members(descs)
    assert [r.tiles_m * r.tiles_n for r in recs] == [0, 2, 0] and recs[0].bytes[2] == 0 and recs[2].bytes[2] == 0
    assert capi.classify_grouped_launches(descs) == 1


def test_refusals():
    L = capi.lib()
    e43 = group("e43", [(3, 5, 7), (65, 33, 100)])
    info = capi.qgemul_info()
    arr = (capi.qgemul_desc * 2)(*e43)
    assert L.qgemul_classify_grouped(arr, 0, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped(arr, -1, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped(None, 2, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped_launches(arr, 0, 0) == capi.QG_EINVAL
    rec = capi.qgemul_grouped_member()
    assert L.qgemul_classify_grouped_member(arr, 2, 0, 2, C.byref(rec)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped_member(arr, 2, 0, -1, C.byref(rec)) == capi.QG_EINVAL
    # a descriptor the plain planner refuses is refused with the same status, wherever it stands in the list
    bad = lower(E43, E43, Qu(4, 3), 3, 5, 7, **L43)
    bad.abi = 77
    st_plain = capi.classify_status(bad)[0]
    assert st_plain != capi.QG_OK
    assert capi.classify_grouped_status([e43[0], bad])[0] == st_plain and capi.classify_grouped_launches([bad, e43[0]]) == st_plain
    # the one-shot call checks its arguments before it touches a device
    Cs = [np.zeros(d.M * d.N, np.int32) for d in e43]
    As = [np.zeros(d.M * d.K, np.int32) for d in e43]
    Bs = [np.zeros(d.K * d.N, np.int32) for d in e43]
    assert capi.run_grouped_status(e43, Cs, As, Bs, flags=capi.OPT_ALL_DEVICES) == capi.QG_EUNSUPPORTED
    assert capi.run_grouped_status(e43, Cs, [As[0], None], Bs) == capi.QG_EINVAL
    assert capi.run_grouped_status(e43, [None, Cs[1]], As, Bs) == capi.QG_EINVAL
    assert capi.run_grouped_status(e43, Cs, As, Bs, ldc=[3, 64]) == capi.QG_EINVAL          # below member 1's 65 rows
    assert capi.run_grouped_status(e43, Cs, As, Bs, lda=[2, 65]) == capi.QG_EINVAL
    assert capi.run_grouped_status(e43, Cs, As, Bs, ldb=[7, 99]) == capi.QG_EINVAL
    assert L.qgemul_run_grouped(arr, 0, None, None, None, None, None, None, None) == capi.QG_EINVAL
