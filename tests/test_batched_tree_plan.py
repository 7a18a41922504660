"""The planner of the one-launch TREE form of batched Qgemul on the CPU (QG_OPT_BATCHED_TREE: a batch whose member runs on a tiled
32-bit tree kernel, tree_i32 or tree_cplx_i32, with a tree of at most 12 levels, as ONE launch of that kernel's batched twin;
qgemul_classify_batched, qgemul_classify_batched_launches: pure host code).  One launch under the flag — three for three members
without it, which is also what a library without the feature answers under the flag —; kernel, class and packed bytes those of the
unflagged plan (the two are interchangeable on the same packed buffers); the unflagged answers restated; everything the flag must not
touch; the workgroup-count limit."""
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, lower, qgemul_epilogue
from stacked_cases import COMPLEX
from test_gpu_tree_levels import REAL

F = capi.OPT_BATCHED_TREE
E88, E43, Q1516 = Qu(8, 8), Qu(4, 3), Qu(15, 16)
C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
I16 = Qu(15, 0, True, TRN.TCPL, WRP.TCPL)
# name -> (element, lowering keywords, kernel, what the member's reason says about its steps)
MEMBERS = {
    "e88": (E88, {}, "tree_i32", b"tree kernel steps: one format, SAT::TCPL, left-justified"),
    "e43": (E43, {}, "tree_i32", b"tree kernel steps: one format, SAT::TCPL, left-justified, packed 16-bit"),
    "q1516": (Q1516, {}, "tree_i32", b"tree kernel steps: one 32-bit format, SAT::TCPL, saturating word adds"),
    "c5_tf": (C5, dict(mul_args=TFComplexMul()), "tree_cplx_i32", b"complex kernel steps: fixed modes, one clamp, packed 16-bit"),
}
SHAPES = [(33, 17, 40), (64, 32, 32), (65, 33, 33), (1, 2, 1), (17, 9, 4096)]   # (one output column of a real member: the one-column kernel, below)


def reason(info):
    return bytes(info.reason).rstrip(b"\0")


@pytest.mark.parametrize("name", sorted(MEMBERS))
def test_one_launch_under_the_flag_three_without(name):
    e, kw, kernel, steps = MEMBERS[name]
    for M, N, K in SHAPES:
        d = lower(e, e, e, M, N, K, **kw)
        plain = capi.classify(d)
        assert capi.KERNEL_NAMES[plain.kernel] == kernel and reason(plain) == b"exact tree evaluation; " + steps
        # without the flag: member by member, the answers this library gave before the form existed
        st, off = capi.classify_batched_status(d, 3)
        assert st == capi.QG_OK and capi.classify_batched_launches(d, 3) == 3
        assert reason(off) == reason(plain) and list(off.packed_bytes) == [3 * ((b + 255) // 256 * 256) for b in plain.packed_bytes]
        for batch in (1, 3, 300):
            st, off = capi.classify_batched_status(d, batch)
            st_on, on = capi.classify_batched_status(d, batch, F)
            assert st == st_on == capi.QG_OK
            assert capi.classify_batched_launches(d, batch) == batch and capi.classify_batched_launches(d, batch, F) == 1, (name, M, N, K, reason(on))
            assert reason(on) == b"batch in one launch; " + steps
            assert on.kernel == off.kernel == plain.kernel and on.cls == off.cls == plain.cls == 2
            assert list(on.packed_bytes) == list(off.packed_bytes) and on.ops == off.ops == batch * plain.ops
            assert list(on.limbs) == list(off.limbs) and on.supported == off.supported == 1


def test_the_pinned_default_stays():
    tree = lower(E88, E88, E88, 33, 17, 40)
    assert capi.classify_batched_launches(tree, 3) == 3
    assert capi.classify_batched_launches(tree, 3, F) == 1
    # the flag next to others: the run-time-mode forms have their twins; the stacked switch does not concern a tree member
    for extra in (capi.OPT_RUNTIME_MODES, capi.OPT_BATCHED_STACKED, capi.OPT_CHECK_RANGE, capi.OPT_GENERIC_LAYOUT):
        st, info = capi.classify_batched_status(tree, 3, F | extra)
        assert st == capi.QG_OK and capi.classify_batched_launches(tree, 3, F | extra) == 1 and reason(info).startswith(b"batch in one launch; ")
        assert capi.classify_batched_launches(tree, 3, extra) == 3
    assert reason(capi.classify_batched_status(tree, 3, F | capi.OPT_RUNTIME_MODES)[1]).endswith(b"tree kernel steps: run-time modes")
    # the general kernel on request: not one of the two kernels with a twin
    st, info = capi.classify_batched_status(tree, 3, F | capi.OPT_GENERIC_TREE)
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == "tree_i64" and capi.classify_batched_launches(tree, 3, F | capi.OPT_GENERIC_TREE) == 3
    # QG_OPT_FORCE_TREE on a linear-class descriptor: a tree_i32 member like any other
    lin = lower(E43, E43, Qu(16, 3), 65, 33, 100, mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
    st, info = capi.classify_batched_status(lin, 3, F | capi.OPT_FORCE_TREE)
    assert st == capi.QG_OK and capi.classify_batched_launches(lin, 3, capi.OPT_FORCE_TREE) == 3
    assert capi.classify_batched_launches(lin, 3, F | capi.OPT_FORCE_TREE) == (1 if capi.KERNEL_NAMES[info.kernel] in ("tree_i32", "tree_cplx_i32") else 3)


def same_answer(d, batch=3):
    a, b = capi.classify_batched_status(d, batch), capi.classify_batched_status(d, batch, F)
    assert a[0] == b[0] and bytes(a[1]) == bytes(b[1]), (a[1].reason, b[1].reason)
    assert capi.classify_batched_launches(d, batch) == capi.classify_batched_launches(d, batch, F)
    assert b"in one launch" not in reason(b[1])
    return a[0], a[1], capi.classify_batched_launches(d, batch)


def test_the_flag_changes_nothing_else():
    # 13 levels: only the 12-level instantiations have a twin
    st, info, n = same_answer(lower(E88, E88, E88, 17, 9, 4097))
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == "tree_i32" and n == 3
    st, info, n = same_answer(lower(C5, C5, C5, 17, 9, 4097, mul_args=TFComplexMul()))
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == "tree_cplx_i32" and n == 3
    # one output column: the one-column kernel
    st, info, n = same_answer(lower(E88, E88, E88, 33, 1, 40))
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == "gemv_i32" and n == 3
    # 64-bit tree values
    ea, ec, kw, flags, kernel, _ = REAL[-1]
    assert kernel == "tree_i64"
    st, info, n = same_answer(lower(ea, ea, ec, 70, 41, 40, **kw))
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == "tree_i64" and n == 3
    # a mixed real x complex tree member: refused as before
    st, info, n = same_answer(lower(E43, C5, Qcomplex(Qu(14, 3), Qu(14, 3)), 33, 17, 40))
    assert st == capi.QG_EUNSUPPORTED and b"mixed real-complex: no batched or grouped plan" in reason(info) and n == capi.QG_EUNSUPPORTED
    # linear class (the block-diagonal MFMA form), a ring member, a complex linear member
    lin = lower(E43, E43, Qu(16, 3), 65, 33, 100, mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
    st, info, n = same_answer(lin)
    assert st == capi.QG_OK and info.cls == 1 and n == 1
    st, info, n = same_answer(lower(I16, I16, I16, 33, 17, 40))
    assert st == capi.QG_OK and b"wrapping ring" in reason(info) and n == 3
    e, ec, kw = COMPLEX["limb2"]
    dc = lower(e, e, ec, 65, 40, 200, **kw)
    st, info, n = same_answer(dc)
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == "mfma_cplx" and n == 6
    # plain plans
    tree = lower(E88, E88, E88, 33, 17, 40)
    for d in (tree, lin, dc):
        assert bytes(capi.classify(d)) == bytes(capi.classify(d, F))
    # chains on batched plans: member by member, with the flag as without
    ep = qgemul_epilogue()
    for d in (tree, lower(C5, C5, C5, 33, 17, 40, mul_args=TFComplexMul()), lin):
        ep.d = d.c[0]
        a, b = capi.classify_batched_epx_status(d, 3, ep), capi.classify_batched_epx_status(d, 3, ep, flags=F)
        assert a[0] == b[0] and bytes(a[1]) == bytes(b[1])
        assert capi.classify_batched_epx_launches(d, 3, ep) == capi.classify_batched_epx_launches(d, 3, ep, flags=F)
        assert b"in one launch" not in reason(b[1])
    st, info = capi.classify_batched_epx_status(tree, 3, ep_for(tree), flags=F)
    assert st == capi.QG_OK and reason(info).startswith(b"chain member by member: ")


def ep_for(d):
    ep = qgemul_epilogue()
    ep.d = d.c[0]
    return ep


def test_a_grouped_plan_ignores_the_flag():
    tree, tall = lower(E88, E88, E88, 33, 17, 40), lower(E88, E88, E88, 70, 41, 64)
    lin = lower(E43, E43, Qu(16, 3), 65, 33, 100, mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
    for group in ([tree, tree], [tree, tall, lin], [lin, lin, tree]):
        a, b = capi.classify_grouped_status(group), capi.classify_grouped_status(group, F)
        assert a[0] == b[0] == capi.QG_OK and bytes(a[1]) == bytes(b[1])
        assert capi.classify_grouped_launches(group) == capi.classify_grouped_launches(group, F)
        for g in range(len(group)):
            assert bytes(capi.classify_grouped_member(group, g)) == bytes(capi.classify_grouped_member(group, g, F))


def test_more_workgroups_than_a_grid_holds_run_member_by_member():
    one = lower(E88, E88, E88, 64, 32, 32)            # one tile per member
    top = 2 ** 31 - 1
    assert capi.classify_batched_launches(one, top, F) == 1
    four = lower(E88, E88, E88, 65, 33, 33)           # 2 x 2 tiles
    assert capi.classify_batched_launches(four, top // 4, F) == 1
    cplx = lower(C5, C5, C5, 65, 33, 33, mul_args=TFComplexMul())   # the packed complex form's tiles have 64 rows too
    assert capi.classify_batched_launches(cplx, top // 4, F) == 1
    for d, batch in ((one, top + 1), (four, top // 4 + 1), (cplx, top // 4 + 1)):
        a, b = capi.classify_batched_status(d, batch), capi.classify_batched_status(d, batch, F)
        assert a[0] == b[0] and bytes(a[1]) == bytes(b[1])
        assert capi.classify_batched_launches(d, batch) == capi.classify_batched_launches(d, batch, F) != 1
    for batch in (0, -1):
        assert capi.classify_batched_status(one, batch, F)[0] == capi.QG_EINVAL


def test_the_binding_has_the_headers_value():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qgemul.h")).read()
    vals = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(QG_OPT_[A-Z_]+) = (\d+)u", hdr)}
    assert vals["QG_OPT_BATCHED_TREE"] == capi.OPT_BATCHED_TREE == 16384
    assert capi.OPT_BATCHED_TREE == 2 * vals["QG_OPT_BATCHED_STACKED"] == max(vals.values())
    assert re.search(r"#define QGEMUL_ABI_VERSION\s+1u\b", hdr)
