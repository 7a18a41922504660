"""The planner of element-wise chains on grouped plans through the built library, without a GPU (the qgemul_classify_grouped_epx*
functions are pure host code): which form runs, the launch counts, where the members of D live, and the refusals.  What needs a
plan (qgemul_packed_e_bytes, the entry points refusing each other, classify against the created plan) is in
tests/test_gpu_grouped_ep.py."""
import ctypes as C

import pytest

import batched_ep_cases as X
import grouped_ep_cases as G
from qublas_amd import capi
from qublas_amd.desc import Approx, Ew, Qcomplex, Qu, RND, SAT, TFComplexMul, Tags, lower, lower_epilogue_x

FUSED, UNFUSED = G.FUSED, G.UNFUSED


def descs_of(fmt, shapes):
    ea, eb, ec, kw, ta, _ = X.FORMATS[fmt]
    return [lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw) for M, N, K in shapes]


def classify(descs, chain, flags=0, per_member="chain"):
    pm = chain.per_member if per_member == "chain" else per_member
    st, info = capi.classify_grouped_epx_status(descs, chain.ep, chain.tabs, pm, flags)
    return st, bytes(info.reason).split(b"\0")[0].decode(), info, capi.classify_grouped_epx_launches(descs, chain.ep, chain.tabs, pm, flags)


def members(descs, chain, flags=0):
    return [capi.classify_grouped_epx_member(descs, chain.ep, g, chain.tabs, chain.per_member, flags) for g in range(len(descs))]


def tiles(d):
    return ((d.M + 63) // 64) * ((d.N + 63) // 64) if d.M and d.N else 0


def test_struct_mirror_matches_the_library():
    assert capi.sizeof(13) == C.sizeof(capi.qgemul_grouped_ep) == 8      # QG_MAX_EW flags and four reserved bytes
    assert capi.SIZEOF_MIRRORS[13] is capi.qgemul_grouped_ep


@pytest.mark.parametrize("chain", G.CHAINS)
@pytest.mark.parametrize("fmt", sorted(X.FORMATS))
def test_all_members_eligible_forms_and_launch_counts(fmt, chain):
    descs = descs_of(fmt, G.SHAPES + G.BIG)
    ch = G.Chain.named(fmt, chain)
    fusable = X.bits32(descs[0], ch.ep, ch.tabs) and not X.has_approx(ch.stages)
    T = sum(tiles(d) for d in descs)
    assert T == 66                                                      # one whole dealt round of 64 and a ragged rest
    for flags in (0, FUSED, UNFUSED, FUSED | UNFUSED):
        st, reason, info, launches = classify(descs, ch, flags)
        fused = fusable and flags == FUSED                              # the pass is the default; QG_OPT_UNFUSED_EPILOGUE forces it
        assert st == capi.QG_OK and launches == (1 if fused else 2), (fmt, chain, flags, reason)
        assert ("chain fused" in reason) == fused and ("chain pass" in reason) == (not fused), reason
        assert "10 members in one launch (66 64x64 tiles)" in reason and "0 run alone" in reason, reason
        assert list(info.limbs) == X.FORMATS[fmt][5]
    if chain.startswith("4_"):
        assert not fusable                                              # not bits32: the pass with and without the flag
    if chain.startswith("5_"):
        assert X.has_approx(ch.stages)                                  # APPROX with the flag falls to the pass


def test_member_offsets_describe_d_and_the_operands_follow_it():
    fmt = "e88_3x3_c16"
    descs = descs_of(fmt, G.SHAPES + G.BIG)
    ch = G.Chain.named(fmt, "4_four_stages_1_2_4_8_bytes")               # D = Qu<20,6>: 4-byte containers after a 2-byte C
    st, reason, info, _ = classify(descs, ch)
    assert st == capi.QG_OK and info.host_elem_bytes[2] == 4
    recs = members(descs, ch)
    end = 0
    for d, r in zip(descs, recs):
        assert r.in_launch == 1 and r.launches == 0
        assert r.off[2] == end and r.bytes[2] == tiles(d) * 4096 * 4     # whole 64 x 64 tiles in D's container, back to back in list order
        end += r.bytes[2]
    assert info.packed_bytes[2] == end
    # A and B are laid out as on the grouped plan without a chain
    plain = [capi.classify_grouped_member(descs, g) for g in range(len(descs))]
    for r, q in zip(recs, plain):
        assert (list(r.off[:2]), list(r.bytes[:2])) == (list(q.off[:2]), list(q.bytes[:2]))


def test_mixed_keys_and_c_formats():
    """the key is that of the first eligible member; with a chain it also compares C's whole format"""
    ch = G.Chain(X.E43, G.MIXED, G.D126)
    e43 = descs_of("e43_c1byte", [(3, 5, 7), (65, 33, 100)])
    e88 = descs_of("e88_3x3_c16", [(65, 33, 100), (3, 5, 7)])
    other_c = lower(X.E43, X.E43, Qu(5, 3), 65, 33, 100, **G.L43)
    # without a chain the Qu<5,3> member shares the launch of the Qu<4,3> ones ...
    same_container = [capi.classify_grouped_member([e43[0], other_c, e43[1]], g).in_launch for g in range(3)]
    descs = [e43[0], e88[0], other_c, e43[1], e88[1]]
    st, reason, _, launches = classify(descs, ch)
    assert st == capi.QG_OK and "2 members in one launch (3 64x64 tiles)" in reason and "3 run alone" in reason
    recs = members(descs, ch)
    assert [r.in_launch for r in recs] == [1, 0, 0, 1, 0]
    # ... (where the conversion into C and the container agree) but never with one
    assert same_container in ([1, 1, 1], [1, 0, 1])
    # a straggler: its kernel (a 3 x 3 pair counts once) and the chain's pass unless its own plain _epx plan fuses
    assert [r.launches for r in recs] == [0, 1, 2, 0, 1]                 # (the 3 x 3-limb plain plan fuses a 32-bit chain by default)
    assert launches == 2 + 1 + 2 + 1
    assert classify(descs, ch, FUSED)[3] == 1 + 1 + 1 + 1                # (single-limb plain plans fuse on request)
    # the stragglers behind the launch's part, 256-byte aligned, in the layout of their own plain _epx plans
    end = recs[0].bytes[2] + recs[3].bytes[2]
    for g in (1, 2, 4):
        st1, info1 = capi.classify_epx(descs[g], ch.ep, ch.tabs)
        assert st1 == capi.QG_OK
        assert recs[g].off[2] == (end + 255) // 256 * 256 and recs[g].bytes[2] == info1.packed_bytes[2]
        end = recs[g].off[2] + recs[g].bytes[2]


@pytest.mark.parametrize("name", sorted(G.STRAGGLERS))
def test_straggler_kinds_carry_the_chain_alone(name):
    a, b, c, kw, shape = G.STRAGGLERS[name]
    ch = G.Chain(X.E43, G.MIXED, G.D126)
    s = lower(a, b, c, *shape, **kw)
    el = descs_of("e43_c1byte", [(3, 5, 7), (65, 33, 100)])
    descs = [el[0], s, s, el[1]]                                         # (an eligible member first: the key is its own)
    st, reason, info, launches = classify(descs, ch)
    assert st == capi.QG_OK and "2 members in one launch" in reason and "2 run alone" in reason, reason
    recs = members(descs, ch)
    assert [r.in_launch for r in recs] == [1, 0, 0, 1]
    assert recs[1].launches == recs[2].launches >= 1 and launches == 2 + 2 * recs[1].launches
    if name == "tree_default_tags":
        assert capi.classify(s).cls == 2 and recs[1].launches == 2       # the tree kernel and the chain's pass


def test_no_member_eligible():
    a, b, c, kw, shape = G.STRAGGLERS["tree_default_tags"]
    ch = G.Chain(X.E88, G.MIXED, G.D126)
    descs = [lower(a, b, c, *shape, **kw), lower(a, b, c, 5, 9, 40, **kw)]
    st, reason, _, launches = classify(descs, ch)
    assert st == capi.QG_OK and "no member eligible, 2 run alone" in reason and launches == 4
    assert [r.in_launch for r in members(descs, ch)] == [0, 0]


def test_identical_descriptors_lay_d_out_as_the_batched_ep_plan_does():
    for fmt in ("e43_c1byte", "e88_3x3_c16", "q78_centred"):
        d = descs_of(fmt, [(65, 33, 100)])[0]
        ch = G.Chain.named(fmt, "1_scale_shared_bias")
        batch = 5
        st, _, info, launches = classify([d] * batch, ch)
        stb, infob = capi.classify_batched_epx_status(d, batch, ch.ep, ch.tabs, [0, 0])
        assert st == stb == capi.QG_OK
        assert list(info.packed_bytes) == list(infob.packed_bytes) and info.host_elem_bytes[2] == infob.host_elem_bytes[2]
        assert launches == capi.classify_batched_epx_launches(d, batch, ch.ep, ch.tabs, [0, 0]) == 2
        recs = members([d] * batch, ch)
        stride = info.packed_bytes[2] // batch
        assert [r.off[2] for r in recs] == [g * stride for g in range(batch)] and all(r.bytes[2] == stride for r in recs)


def test_status_is_any_member_descriptors_own_wherever_it_stands():
    ch = G.Chain(X.E43, G.MIXED, G.D126)
    el = descs_of("e43_c1byte", [(3, 5, 7), (65, 33, 100)])
    C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))
    cx = lower(C5, C5, C5, 5, 9, 40, mul_args=TFComplexMul())
    want, winfo = capi.classify_epx(cx, ch.ep, ch.tabs)
    assert want != capi.QG_OK
    for descs in ([cx] + el, [el[0], cx, el[1]], el + [cx]):
        st, reason, _, launches = classify(descs, ch)
        assert st == want == launches and reason == bytes(winfo.reason).split(b"\0")[0].decode()
    # a chain that no member's C supports: the status of qgemul_classify_epx
    bad = G.Chain(X.E43, [Ew("mul", Qu(30, 20), scalar=True), Ew("mul", Qu(30, 20), scalar=True), Ew("mul", Qu(30, 20), scalar=True)], Qu(60, 3))
    st1, _ = capi.classify_epx(el[0], bad.ep, bad.tabs)
    assert classify(el, bad)[0] == st1


def test_einval_without_a_device():
    ch = G.Chain.named("e43_c1byte", "5_act_uniform")                    # scalar mul, tensor add, APPROX
    el = descs_of("e43_c1byte", [(3, 5, 7), (65, 33, 100)])
    assert classify(el, ch, per_member=[1, 0, 0])[0] == capi.QG_OK
    assert classify(el, ch, per_member=None)[0] == capi.QG_OK            # NULL: no stage is per member
    for bad in ([0, 1, 0], [0, 0, 1], [1, 0, 0, 1]):                      # a tensor stage, an APPROX stage, a stage the chain does not have
        st, reason, _, launches = classify(el, ch, per_member=bad)
        assert st == capi.QG_EINVAL == launches and "scalar_per_member" in reason, (bad, reason)
    L = capi.lib()
    info = capi.qgemul_info()
    arr = capi._desc_array(el)
    assert L.qgemul_classify_grouped_epx(arr, 0, C.byref(ch.ep), None, None, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped_epx(None, 2, C.byref(ch.ep), None, None, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped_epx(arr, 2, None, None, None, 0, C.byref(info)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped_epx(arr, 2, C.byref(ch.ep), None, None, 0, None) == capi.QG_EINVAL
    rec = capi.qgemul_grouped_member()
    assert L.qgemul_classify_grouped_epx_member(arr, 2, C.byref(ch.ep), capi._tables(ch.tabs), None, 0, 2, C.byref(rec)) == capi.QG_EINVAL
    assert L.qgemul_classify_grouped_epx_member(arr, 2, C.byref(ch.ep), capi._tables(ch.tabs), None, 0, -1, C.byref(rec)) == capi.QG_EINVAL
    # an APPROX stage without its table is refused as qgemul_classify_epx refuses it
    assert L.qgemul_classify_grouped_epx(arr, 2, C.byref(ch.ep), None, None, 0, C.byref(info)) == L.qgemul_classify_epx(C.byref(el[0]), C.byref(ch.ep), capi._tables([]), 0, C.byref(info)) != capi.QG_OK


def test_the_plan_without_a_chain_is_what_it_was():
    descs = descs_of("e88_3x3", G.SHAPES + G.BIG)
    st, info = capi.classify_grouped_status(descs)
    assert st == capi.QG_OK and b"10 members in one launch (66 64x64 tiles), 0 run alone" in bytes(info.reason)
    assert capi.classify_grouped_launches(descs) == 1
