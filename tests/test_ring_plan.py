"""Which descriptors are ring plans (qublas_amd/csrc/qg_plan.cpp: ring_plan; qg_geom.cpp: qg_plan_geometry).  Product and every tree level
in ONE signed WRP::TCPL format of n <= 32 bits, entered by an exact left shift: the linear class on the int8 matrix cores, with the
limb products of weight below 2^n only and no bound on K.  The neighbours — anything that rounds or clamps between the additions —
keep the tree kernels they had, asserted by kernel name.  CPU only: classification needs no GPU."""
import pytest

import golden_io as G
from qublas_amd import capi
from qublas_amd.desc import BasicComplexMul, CLASS_LINEAR, CLASS_TREE, Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, desc_from_dict, lower


def I(bits):
    return Qu(bits - 1, 0, True, TRN.TCPL, WRP.TCPL)


def R(i, f, q=TRN.TCPL):
    return Qu(i, f, True, q, WRP.TCPL)


def ring_kw(r):
    return dict(mul_args=Tags.of(r), add_args=[r])


def plan(d, flags=0):
    info = capi.classify(d, flags)
    return capi.KERNEL_NAMES[info.kernel], info.cls, tuple(info.limbs), bytes(info.reason).split(b"\0")[0].decode()


RINGS = [
    # name, descriptor, kernel, limbs, n, products
    ("int8", lower(I(8), I(8), I(8), 300, 200, 1000), "mfma_i8", (1, 1), 8, 1),
    ("int12", lower(I(12), I(12), I(12), 300, 200, 1000), "mfma_i8_limb", (2, 2), 12, 3),
    ("int16", lower(I(16), I(16), I(16), 300, 200, 1000), "mfma_i8_limb", (2, 2), 16, 3),
    ("int24", lower(I(24), I(24), I(24), 300, 200, 1000), "mfma_i8_limb", (3, 3), 24, 6),
    ("int32", lower(I(32), I(32), I(32), 300, 200, 1000), "mfma_i8_limb", (4, 4), 32, 10),
    ("int32, K = 1", lower(I(32), I(32), I(32), 300, 200, 1), "mfma_i8_limb", (4, 4), 32, 10),
    ("int32, one column", lower(I(32), I(32), I(32), 300, 1, 4096), "mfma_i8_limb", (4, 4), 32, 10),
    ("int8 x int16 into an explicit int24 ring", lower(I(8), I(16), I(24), 64, 64, 500, **ring_kw(I(24))), "mfma_i8_limb", (1, 3), 24, 3),
    ("int12 x int32 into an explicit int32 ring", lower(I(12), I(32), I(32), 64, 64, 500, **ring_kw(I(32))), "mfma_i8_limb", (2, 4), 32, 7),
    ("saturating operands into an int16 ring", lower(Qu(15, 0), Qu(15, 0), I(16), 64, 64, 37, **ring_kw(I(16))), "mfma_i8_limb", (2, 2), 16, 3),
    ("left shift 2: int16 into Qu<13,2>", lower(I(16), I(16), Qu(20, 4), 64, 64, 37, **ring_kw(R(13, 2))), "mfma_i8_limb", (2, 2), 16, 3),
    ("left shift 15 of 16", lower(I(8), I(8), R(0, 15), 64, 64, 37, **ring_kw(R(0, 15))), "mfma_i8_limb", (1, 1), 16, 1),
    ("saturating C", lower(I(16), I(16), Qu(7, 0), 64, 64, 37), "mfma_i8_limb", (2, 2), 16, 3),
    ("rounded C", lower(Qu(7, 1), Qu(7, 1), Qu(10, 0, True, RND.CONV, SAT.SMGN), 64, 64, 37, **ring_kw(R(13, 2))), "mfma_i8_limb", (2, 2), 16, 3),
    ("C wider than the ring", lower(I(32), I(32), Qu(40, 4), 64, 64, 37), "mfma_i8_limb", (4, 4), 32, 10),
    ("levels of another QuMode", lower(I(24), I(24), I(24), 64, 64, 37, mul_args=Tags.of(I(24)), add_args=[R(23, 0, RND.POS_INF)]), "mfma_i8_limb", (3, 3), 24, 6),
    ("int8, K = 2^20 in one launch", lower(I(8), I(8), I(8), 128, 128, 1 << 20), "mfma_i8", (1, 1), 8, 1),
    ("int8 operands, int32 ring, K = 2^18", lower(I(8), I(8), I(32), 32, 16, 1 << 18, **ring_kw(I(32))), "mfma_i8_limb", (1, 1), 32, 1),
]


@pytest.mark.parametrize("name,d,kernel,limbs,n,products", RINGS, ids=[r[0] for r in RINGS])
def test_ring_descriptors_take_the_matrix_cores(name, d, kernel, limbs, n, products):
    k, cls, lm, reason = plan(d)
    assert (k, cls, lm) == (kernel, CLASS_LINEAR, limbs), (k, cls, lm, reason)
    assert reason == "linear class: wrapping ring mod 2^%d, %d limb product%s" % (n, products, "" if products == 1 else "s")
    assert "k-chunk" not in reason
    # QG_OPT_FORCE_TREE: the tree plan such a descriptor had before
    kt, _, lt, rt = plan(d, capi.OPT_FORCE_TREE)
    assert kt in ("tree_i32", "tree_i64", "tree_i128", "gemv_i32", "gemv_i64") and lt == (0, 0) and "ring" not in rt, (kt, rt)


def test_forced_tree_kernels_are_the_backstops_the_ring_replaces():
    for bits, tree in ((8, "tree_i32"), (12, "tree_i32"), (16, "tree_i64"), (24, "tree_i64"), (32, "tree_i128")):
        d = lower(I(bits), I(bits), I(bits), 128, 128, 4096)
        assert plan(d, capi.OPT_FORCE_TREE)[0] == tree
        assert "wrapping ring" in plan(d)[3]
    assert plan(lower(I(8), I(8), I(8), 128, 128, 262144), capi.OPT_FORCE_TREE)[0] == "tree_i64"


Q1516 = Qu(15, 16, True, TRN.TCPL, WRP.TCPL)
NEIGHBOURS = [
    # name, descriptor, the kernel it keeps
    ("d > 0: Q15.16 words that wrap", lower(Q1516, Q1516, Q1516, 128, 128, 4096), "tree_i32"),
    ("d > 0: int<8,8> product rounded into a 16-bit ring", lower(R(7, 8), R(7, 8), R(7, 8), 128, 128, 4096), "tree_i32"),
    ("a saturating level", lower(I(16), I(16), I(16), 128, 128, 4096, mul_args=Tags.of(I(16)), add_args=[I(16), Qu(15, 0), I(16)]), "tree_i64"),
    ("a saturating product", lower(I(16), I(16), I(16), 128, 128, 4096, mul_args=Tags.of(Qu(15, 0)), add_args=[I(16)]), "tree_i64"),
    ("one level of another width", lower(I(16), I(16), I(16), 128, 128, 4096, mul_args=Tags.of(I(16)), add_args=[I(16), I(20), I(16)]), "tree_i64"),
    ("one level with other fraction bits", lower(I(16), I(16), I(16), 128, 128, 4096, mul_args=Tags.of(I(16)), add_args=[I(16), R(14, 1), I(16)]), "tree_i64"),
    ("an unsigned ring", lower(Qu(16, 0, False, TRN.TCPL, WRP.TCPL), Qu(16, 0, False, TRN.TCPL, WRP.TCPL), Qu(16, 0, False, TRN.TCPL, WRP.TCPL), 128, 128, 4096), "tree_i64"),
    ("a ring of 33 bits", lower(I(32), I(32), I(33), 128, 128, 4096, **ring_kw(I(33))), "tree_i128"),
    ("one column the 32-bit one-column kernel walks", lower(I(8), I(8), I(8), 300, 1, 4096), "gemv_i32"),
    ("one column the 64-bit one-column kernel walks", lower(I(16), I(16), I(16), 300, 1, 4096), "gemv_i64"),
]


@pytest.mark.parametrize("name,d,kernel", NEIGHBOURS, ids=[n[0] for n in NEIGHBOURS])
def test_neighbours_keep_their_plans(name, d, kernel):
    k, cls, limbs, reason = plan(d)
    assert k == kernel and cls == CLASS_TREE and limbs == (0, 0) and "ring" not in reason, (k, cls, reason)


def test_complex_descriptors_keep_their_plans():
    c = Qcomplex(I(16), I(16))
    d = lower(c, c, c, 128, 128, 4096, mul_args=BasicComplexMul())
    k, cls, _, reason = plan(d)
    assert k in ("tree_cplx", "tree_cplx_i32") and cls == CLASS_TREE and "ring" not in reason


def test_unsigned_32_bit_ring_stays_refused():
    u = Qu(32, 0, False, TRN.TCPL, WRP.TCPL)
    st, info = capi.classify_status(lower(u, u, u, 128, 128, 4096))
    assert st != 0 and not info.supported and b"allOnes" in bytes(info.reason)


def test_exact_descriptors_keep_the_exact_linear_plan():
    """operands so narrow that nothing can wrap: the plain linear class, with its own kernels"""
    d = lower(I(4), I(4), I(32), 128, 128, 4096, **ring_kw(I(32)))
    k, cls, limbs, reason = plan(d)
    assert k == "mfma_i8" and cls == CLASS_LINEAR and "ring" not in reason


def test_every_fixture_record_is_a_ring_plan():
    recs = list(G._records(G.GOLD + "/ref_ring_0.jsonl.gz"))
    assert len(recs) == 17
    for j in recs:
        k, cls, _, reason = plan(desc_from_dict(j))
        assert k in ("mfma_i8", "mfma_i8_limb") and cls == CLASS_LINEAR and "wrapping ring" in reason, (j["name"], k, reason)


def test_no_committed_gemm_record_changes_class():
    for j in G.gemm_cases("real") + G.gemm_cases("cplx"):
        st, info = capi.classify_status(desc_from_dict(j))
        assert b"wrapping ring" not in bytes(info.reason), j["name"]
