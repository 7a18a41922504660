"""Kernels at edge operands (dist 2: oracle/qoracle.c qo_edges — lo, lo + 1, -one - 1 ... one + 1, hi - 1, hi of every format,
about half of all elements): exact boundary products (-1 * min, 1 * max, (1 + ulp) * max), rounding ties (1/2 * odd) and
boundary node sums in every reduction of a few dozen leaves.
 - the reference's own dist-2 records (tests/golden/ref_gemm_*), also under the run-time-mode and generic tree kernels;
 - every step form against the oracle on shapes that straddle the kernels' tiles and k-chunks, with witnesses that the
   case is not vacuous (a boundary product, a tie where the product rounds, saturated and unsaturated outputs);
 - an element-wise chain into the widest format the chain kernels take (62 value bits)."""
import numpy as np
import pytest

import golden_io as G
from qublas_amd import capi
from qublas_amd.desc import (BasicComplexMul, Ew, Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, desc_from_dict, lower,
                             lower_epilogue, lower_reduce, reduce_result_type)

pytestmark = pytest.mark.gpu

EDGE_RECORDS = [j for j in G.gemm_cases("real") + G.gemm_cases("cplx")
                if j["inputs"].get("dist", j["inputs"].get("from", {}).get("dist")) == 2]


def run(d, A, B, ec, oracle, flags=0):
    return capi.run(d, np.zeros(d.M * d.N, dtype=oracle.host_dtype(ec)), A, B, flags=flags)


def same(a, b):
    if a.dtype.names:
        return all(np.array_equal(a[n], b[n]) for n in a.dtype.names)
    return np.array_equal(a, b)


@pytest.mark.parametrize("j", EDGE_RECORDS, ids=lambda j: j["name"])
def test_edge_records_second_opinions(oracle, j):
    """each dist-2 reference record (its default plan runs in test_gpu_parity.py::test_golden_vectors) on the run-time-mode
    kernels and the generic tree kernel, and linear ones on the exact tree kernel: all must give the reference's C"""
    d = desc_from_dict(j)
    A, B = G.case_inputs(j, oracle)
    _, _, ec = G.case_elems(j)
    exp = G.case_expected(j, oracle)
    flags = [capi.OPT_RUNTIME_MODES, capi.OPT_GENERIC_TREE]
    if capi.KERNEL_NAMES[capi.classify(d).kernel].startswith("mfma"):
        flags.append(capi.OPT_FORCE_TREE)
    for fl in flags:
        assert same(run(d, A, B, ec, oracle, flags=fl), exp), (j["name"], fl)


def witnesses(A, B, ea, eb, pf, ec, M, N, K, ta, got):
    """numpy, from the operands: where the product keeps the operands' format, some product quantises to its boundary (lo - 1,
    lo, hi, hi + 1 before overflow handling), else some product overflows the product format; a product that is an exact
    rounding tie where the product shifts right and rounds; where C is the product's format and saturates, some outputs
    saturated and (signed formats: unsigned sums of full-range values saturate by nature) at least 10 % not"""
    a = A.astype(object).reshape(M, K) if ta else A.astype(object).reshape(M, K, order="F")   # (i, k) at k + i K / i + k M
    b = B.astype(object).reshape(K, N, order="F")
    p = (a[:, :, None] * b[None, :, :min(N, 4)]).ravel()            # exact products (the first columns)
    d = ea.fracBits + eb.fracBits - pf.fracBits
    q = [v >> d if d >= 0 else v << -d for v in p]
    if (pf.intBits, pf.fracBits) == (ea.intBits, ea.fracBits):
        edges = {pf.raw_min - 1, pf.raw_min, pf.raw_max, pf.raw_max + 1}
        assert any(v in edges for v in q), "no boundary product"
    else:
        assert any(v < pf.raw_min or v > pf.raw_max for v in q), "no product overflows"
    if d >= 1 and pf.QuMode != TRN.TCPL:
        assert any(v % (1 << d) == 1 << (d - 1) for v in p), "no rounding tie"
    if (ec.intBits, ec.fracBits) == (pf.intBits, pf.fracBits) and ec.OfMode in (SAT.TCPL, SAT.SMGN):
        g = got.astype(np.int64)
        sat = (g == ec.raw_max) | (g == ec.raw_min)
        assert sat.any(), "no saturated output"
        assert not ec.isSigned or (~sat).mean() >= 0.1, "(almost) every output saturated"


P = lambda i, f: Qu(i, f, True, RND.POS_INF, SAT.TCPL)
C5 = Qcomplex(P(6, 3), P(6, -3))
Q1516 = Qu(15, 16)
# (A, B, C, lowering keywords, product format (checked against the lowering), kernel, step form — the form at every shape
# is pinned through the planner driver by tests/test_form_coverage.py::test_gpu_edge_cases_reach_their_forms)
REAL = [
    (Qu(0, 31), Qu(0, 31), Qu(0, 31), {}, Qu(0, 31), "tree_i32", "QTF_WORD"),                                                    # shift 31
    (Qu(7, 24), Qu(7, 24), Qu(7, 24), {}, Qu(7, 24), "tree_i32", "QTF_WORD"),                                                    # shift 24
    (Q1516, Q1516, Q1516, {}, Q1516, "tree_i32", "QTF_WORD_MAD"),
    (Qu(1, 28), Qu(1, 28), Qu(1, 28), {}, Qu(1, 28), "tree_i32", "QTF_JWORD"),
    (Qu(11, 12), Qu(11, 12), Qu(11, 12), {}, Qu(11, 12), "tree_i32", "QTF_JWORD"),
    (Qu(14, 16), Qu(14, 16), Qu(14, 16), {}, Qu(14, 16), "tree_i32", "QTF_JWORD_MAD"),
    (Qu(15, 16, True, TRN.TCPL, WRP.TCPL),) * 3 + ({}, Qu(15, 16, True, TRN.TCPL, WRP.TCPL), "tree_i32", "QTF_WORD_WRAP"),
    (Qu(6, 5), Qu(6, 5), Qu(9, 2), dict(mul_args=Qu(7, 6, True, RND.NEG_INF, SAT.TCPL), add_args=[Qu(7, 6)]), Qu(7, 6, True, RND.NEG_INF), "tree_i32", "QTF_PK16_HYB"),
    (Qu(7, 8), Qu(7, 8), Qu(7, 8), {}, Qu(7, 8), "tree_i32", "QTF_PK16_HYB16"),
    (P(7, 8), P(7, 8), Qu(12, 4), {}, P(7, 8), "tree_i32", "QTF_PK16_HYB16"),                                                          # ... rounding products
    (Qu(12, 5, False),) * 3 + ({}, Qu(12, 5, False), "tree_i32", "QTF_LJ_U"),
    (Qu(8, 0, False),) * 3 + ({}, Qu(8, 0, False), "tree_i32", "QTF_PK16_U"),
    (Qu(7, 6, False), Qu(7, 6, False), Qu(9, 2, False), dict(mul_args=Qu(8, 6, False, RND.NEG_INF, SAT.TCPL), add_args=[Qu(8, 6, False)]),
     Qu(8, 6, False, RND.NEG_INF), "tree_i32", "QTF_PK16_HYB_U"),
    (Qu(8, 8, False),) * 3 + ({}, Qu(8, 8, False), "tree_i32", "QTF_PK16_HYB16_U"),
    (Qu(8, 8),) * 3 + ({}, Qu(8, 8), "tree_i32", "QTF_LJ"),
    (Qu(4, 3),) * 3 + ({}, Qu(4, 3), "tree_i32", "QTF_PK16"),
    (Qu(4, 3), Qu(4, 3), Qu(9, 2), dict(mul_args=P(5, 4), add_args=[Qu(5, 4)]), P(5, 4), "tree_i32", "QTF_PK16"),                  # ... rounding products (ties)
    (Qu(5, 4, False), Qu(5, 4, False), Qu(9, 2, False), dict(mul_args=Qu(7, 4, False, RND.POS_INF, SAT.TCPL), add_args=[Qu(7, 4, False)]),
     Qu(7, 4, False, RND.POS_INF), "tree_i32", "QTF_PK16_U"),                                                                       # rounding products
    (Qu(8, 8, True, TRN.TCPL, SAT.ZERO),) * 3 + ({}, Qu(8, 8, True, TRN.TCPL, SAT.ZERO), "tree_i32", "QTF_ONE_ZERO"),
    (Qu(4, 3), Qu(4, 3), Qu(8, 6, False), dict(mul_args=Qu(8, 6, False), add_args=[Qu(8, 6, False)]), Qu(8, 6, False), "tree_i32", "QTF_ONE_TCPL"),
    (Qu(8, 8), Qu(8, 8), Qu(12, 8), dict(add_args=[Qu(12, 8)]), Qu(8, 8), "tree_i32", "QTF_REC_CLAMP"),
    (Qu(8, 8, True, TRN.TCPL, SAT.ZERO),) * 2 + (Qu(12, 6, True, TRN.TCPL, SAT.ZERO),
     dict(add_args=[Qu(10, 8, True, TRN.TCPL, SAT.ZERO), Qu(12, 6, True, TRN.TCPL, SAT.ZERO)]), Qu(8, 8, True, TRN.TCPL, SAT.ZERO), "tree_i32", "QTF_REC_BIASED"),
    (Qu(8, 8), Qu(8, 8), Qu(12, 8), dict(add_args=[Qu(12, 8, True, RND.CONV)], mul_args=Qu(10, 6, True, RND.CONV)), Qu(10, 6, True, RND.CONV), "tree_i32", "QTF_REC_KINDS"),
    (Qu(15, 16, True, TRN.TCPL, SAT.ZERO),) * 3 + ({}, Qu(15, 16, True, TRN.TCPL, SAT.ZERO), "tree_i64", None),            # 64-bit tree kernel
]
# one column: (element, level types, [(rows, K)], kernel, form as a GEMV, form as a Qreduce (a 0/1 vector)) on the one-column kernels
T1, T2 = Qu(6, 5, True, RND.CONV, SAT.SMGN), Qu(8, 4, True, RND.ZERO, SAT.TCPL)
COLUMN = [
    (Q1516, None, [(129, 257), (65, 513)], "gemv_i32", "QGF_WORD_RND", "QGF_WORD"),
    (Qu(8, 8, True, TRN.TCPL, SAT.ZERO), None, [(129, 33), (65, 513)], "gemv_i32", "QGF_ONE_ZERO", "QGF_ONE_ZERO"),
    (Qu(4, 3), None, [(127, 31), (64, 512)], "gemv_i32", "QGF_ONE_TCPL", "QGF_ONE_TCPL"),
    (Qu(8, 8), [Qu(10, 8), Qu(12, 8)], [(129, 33), (65, 513)], "gemv_i32", "QGF_REC_CLAMP", "QGF_REC_CLAMP"),
    (Qu(4, 3), [T1, T2], [(127, 31), (64, 512)], "gemv_i32", "QGF_REC_KINDS", "QGF_REC_KINDS"),
    (Qu(15, 16, True, TRN.TCPL, WRP.TCPL), None, [(63, 33), (65, 511)], "gemv_i64", None, None),   # the 64-bit one-column kernel
]


def column_cases(e, levels, rows, K, oracle):
    """(descriptor, B, C) of the GEMV and of the Qreduce"""
    ec = reduce_result_type(e, levels or [], K)
    gemv = lower(e, e, levels[-1] if levels else e, rows, 1, K, add_args=levels)
    return [(gemv, oracle.fill(e, K, 44, 2) if oracle else None, levels[-1] if levels else e),
            (lower_reduce(e, rows, K, levels), np.ones(K, dtype=np.int32), ec)]


# (element, C, lowering keywords, step form)
CPLX = [
    (C5, C5, dict(mul_args=TFComplexMul()), "QCF_PK16"),
    (C5, C5, dict(mul_args=TFComplexMul(ABT=Tags(7, 3))), "QCF_COMPACT"),
    (Qcomplex(P(8, 4), P(8, 4)), C5, dict(mul_args=TFComplexMul()), "QCF_LJ"),
    (Qcomplex(Qu(6, 3, True, RND.NEG_INF, SAT.SMGN), Qu(6, 3, True, RND.NEG_INF, SAT.SMGN)), C5, dict(mul_args=BasicComplexMul()), "QCF_UNIFORM"),
    (C5, Qcomplex(P(12, 4), P(10, 2)), dict(mul_args=BasicComplexMul(acT=Tags(20, 8))), "QCF_TABLE"),
    (Qcomplex(Qu(6, 3, True, RND.CONV), Qu(6, 3, True, RND.CONV)), Qcomplex(Qu(9, 3), Qu(9, 1)), dict(mul_args=TFComplexMul()), "QCF_KINDS_R"),
    (Qcomplex(Qu(6, 3, True, TRN.TCPL, SAT.ZERO), Qu(6, -3, True, TRN.TCPL, SAT.ZERO)),
     Qcomplex(Qu(9, 3, True, TRN.TCPL, SAT.ZERO), Qu(9, 1, True, TRN.TCPL, SAT.ZERO)), dict(mul_args=TFComplexMul()), "QCF_KINDS_Z"),
    (Qcomplex(Qu(6, 3, True, RND.CONV, SAT.ZERO), Qu(6, 3, True, RND.CONV, SAT.ZERO)), Qcomplex(Qu(9, 3), Qu(9, 1)), dict(mul_args=TFComplexMul()), "QCF_KINDS_RZ"),
    (Qcomplex(Qu(6, 3, True, TRN.TCPL, WRP.TCPL), Qu(6, 1, True, TRN.TCPL, WRP.TCPL)),
     Qcomplex(Qu(7, 3, True, TRN.TCPL, WRP.TCPL), Qu(5, 1, True, TRN.TCPL, WRP.TCPL)), dict(mul_args=TFComplexMul()), "QCF_KINDS_W"),
    (Qcomplex(Qu(6, 3, True, RND.CONV, WRP.TCPL), Qu(6, 3, True, RND.CONV, WRP.TCPL)), Qcomplex(Qu(9, 3), Qu(9, 1)), dict(mul_args=TFComplexMul()), "QCF_KINDS_RW"),
    (Qcomplex(Qu(6, 3, True, RND.INF), Qu(6, 1, True, RND.INF, SAT.ZERO)), Qcomplex(Qu(7, 1, True, RND.INF), Qu(5, 0, True, RND.INF, WRP.TCPL)),
     dict(mul_args=BasicComplexMul(acT=Tags(8, 4)), add_args=[Qcomplex(Qu(12, 2, True, RND.INF), Qu(12, 1, True, RND.INF, SAT.ZERO))]), "QCF_KINDS_ALL"),
    (Qcomplex(Qu(5, 4, True, RND.INF, WRP.TCPL), Qu(6, 2, False, RND.ZERO, WRP.TCPL)), Qcomplex(Qu(6, 2, True, RND.INF, SAT.ZERO), Qu(5, 1, False, RND.CONV, WRP.TCPL)),
     dict(mul_args=TFComplexMul(), add_args=[Qcomplex(Qu(9, 3, True, RND.INF, WRP.TCPL), Qu(8, 1, False, TRN.SMGN, WRP.TCPL)),
                                             Qcomplex(Qu(7, 2, True, RND.ZERO, SAT.ZERO), Qu(9, 3, True, RND.CONV, SAT.SMGN))]), "QCF_KINDS"),
]
SHAPES = [(65, 63, 33), (129, 127, 513), (64, 128, 31)]


@pytest.mark.parametrize("case", range(len(REAL)))
def test_real_forms_at_edge_operands(oracle, case):
    ea, eb, ec, kw, pf, kernel, _ = REAL[case]
    for M, N, K in SHAPES:
        ta = K == 513
        d = lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)
        assert capi.KERNEL_NAMES[capi.classify(d).kernel] == kernel, (str(ea), capi.classify(d).reason)
        m = d.mul[0]
        assert (m.I, m.F, m.S, m.Q, m.O) == (pf.intBits, pf.fracBits, int(pf.isSigned), pf.QuMode, pf.OfMode), str(pf)
        A, B = oracle.fill(ea, M * K, 41, 2), oracle.fill(eb, K * N, 42, 2)
        got = run(d, A, B, ec, oracle)
        exp = oracle.gemm(d, A, B, ec, nthreads=8)
        assert np.array_equal(got, exp), (str(ea), M, N, K)
        assert np.array_equal(run(d, A, B, ec, oracle, flags=capi.OPT_RUNTIME_MODES), exp)
        witnesses(A, B, ea, eb, pf, ec, M, N, K, ta, got)


@pytest.mark.parametrize("case", range(len(COLUMN)))
def test_one_column_forms_at_edge_operands(oracle, case):
    e, levels, shapes, kernel, _, _ = COLUMN[case]
    for rows, K in shapes:
        for d, B, ec in column_cases(e, levels, rows, K, oracle):
            assert capi.KERNEL_NAMES[capi.classify(d).kernel] == kernel, (str(e), K, capi.classify(d).reason)
            A = oracle.fill(e, rows * K, 43, 2)
            got = run(d, A, B, ec, oracle)
            exp = oracle.gemm(d, A, B, ec, nthreads=8)
            assert np.array_equal(got, exp), (str(e), rows, K)
            assert np.array_equal(run(d, A, B, ec, oracle, flags=capi.OPT_RUNTIME_MODES), exp)
            sat = (got.astype(np.int64) == ec.raw_max) | (got.astype(np.int64) == ec.raw_min)
            assert (~sat).mean() >= 0.1 and (sat.any() or levels or ec.OfMode != SAT.TCPL)   # (level types: C is wider than the nodes)


@pytest.mark.parametrize("case", range(len(CPLX)))
def test_complex_forms_at_edge_operands(oracle, case):
    e, ec, kw, _ = CPLX[case]
    for M, N, K in SHAPES:
        d = lower(e, e, ec, M, N, K, transposed_a=K == 513, **kw)
        assert capi.KERNEL_NAMES[capi.classify(d).kernel] == "tree_cplx_i32", capi.classify(d).reason
        A, B = oracle.fill(e, M * K, 45, 2), oracle.fill(e, K * N, 46, 2)
        got = run(d, A, B, ec, oracle)
        exp = oracle.gemm(d, A, B, ec, nthreads=8)
        assert same(got, exp), (M, N, K)
        assert same(run(d, A, B, ec, oracle, flags=capi.OPT_RUNTIME_MODES), exp)
        for part, f in (("re", ec.real), ("im", ec.imag)):   # (saturating signed parts: >= 10 % unsaturated where K is short, some where long)
            g = got[part].astype(np.int64)
            if f.isSigned and f.OfMode in (SAT.TCPL, SAT.SMGN):
                assert ((g != f.raw_max) & (g != f.raw_min)).mean() >= (0.1 if K <= 33 else 0.01), (part, M, N, K)
        # edges in the operands: the parts' minima and maxima are all there
        assert (A["re"] == e.real.raw_min).any() and (A["im"] == e.imag.raw_max).any()


CENTRED = [
    # (A = B, C, lowering keywords, limbs) — narrow C: the epilogue rounds and saturates
    (Qu(7, 8), Qu(9, 3, True, RND.CONV, SAT.SMGN), dict(mul_args=Tags(15, 16), add_args=[Qu(28, 16)]), [2, 2]),
    (Qu(8, 0, False), Qu(12, -4, False, RND.CONV, SAT.SMGN), dict(mul_args=Tags(16, 0, False), add_args=[Qu(28, 0, False)]), [1, 1]),
    (Qu(11, 12), Qu(20, 8, True, RND.CONV, SAT.SMGN), dict(mul_args=Tags(23, 24), add_args=[Qu(35, 24)]), [3, 3]),
]


@pytest.mark.parametrize("case", range(len(CENTRED)))
def test_centred_plans_at_edge_operands(oracle, case):
    e, ec, kw, limbs = CENTRED[case]
    for M, N, K in ((65, 63, 33), (129, 127, 511), (64, 65, 513)):
        d = lower(e, e, ec, M, N, K, **kw)
        assert list(capi.classify(d).limbs) == limbs
        A, B = oracle.fill(e, M * K, 47, 2), oracle.fill(e, K * N, 48, 2)
        got = run(d, A, B, ec, oracle)
        assert np.array_equal(got, oracle.gemm(d, A, B, ec, nthreads=8)), (M, N, K)
        assert got.tobytes() == run(d, A, B, ec, oracle, flags=capi.OPT_BALANCED_LIMBS).tobytes()
        sat = (got.astype(np.int64) == ec.raw_max) | (got.astype(np.int64) == ec.raw_min)
        assert sat.any() and (not ec.isSigned or (~sat).mean() >= 0.1)


@pytest.mark.parametrize("case", [0, 1])
def test_k_chunked_plans_at_edge_operands(oracle, case):
    """K beyond one launch: the composite plan's k-chunks (single limb / centred 2 x 2 limbs), each chunk's partial sums
    combined exactly in 64 bits, with edge operands in every chunk"""
    e, ec, kw, K = [(Qu(8, 0, False), Qu(30, 0, False), dict(mul_args=Tags(16, 0, False), add_args=[Qu(34, 0, False)]), 140001),
                    (Qu(7, 8), Qu(30, 8), dict(mul_args=Tags(15, 16), add_args=[Qu(33, 16)]), 70001)][case]
    M, N = 33, 17
    d = lower(e, e, ec, M, N, K, **kw)
    info = capi.classify(d)
    assert capi.KERNEL_NAMES[info.kernel].startswith("mfma") and "chunk(s)" in info.reason.decode(), info.reason
    A, B = oracle.fill(e, M * K, 49, 2), oracle.fill(e, K * N, 50, 2)
    assert (A == e.raw_min).any() and (A == e.raw_max).any() and (B == e.raw_max).any()
    got = run(d, A, B, ec, oracle)
    assert np.array_equal(got, oracle.gemm(d, A, B, ec, nthreads=8))


def test_element_wise_chain_into_62_bits(oracle):
    """the widest formats the 64-bit chain kernels take, at edge operands: a product of the 41-bit C and a 21-bit tensor
    into a stage result of 62 value bits (|value| up to 2^60), then into D = Qu<62,0> and, saturating, into Qu<50,0>.
    (No accepted chain can exceed Qu<62,0>'s own range: every intermediate is bounded by 62 bits, so a conversion into a
    62-bit format never overflows; tests/test_eltwise.py checks that wider formats are refused.)"""
    e, c, s = Qu(20, 0), Qu(40, 0), Qu(20, 0)
    M, N, K = 65, 33, 37
    d = lower(e, e, c, M, N, K, mul_args=Tags(40, 0), add_args=[Qu(40, 0)])
    A, B = oracle.fill(e, M * K, 51, 2), oracle.fill(e, K * N, 52, 2)
    E = [oracle.fill(s, M * N, 53, 2)]
    C = oracle.gemm(d, A, B, c, nthreads=8).astype(np.int64)
    for D in (Qu(62, 0), Qu(50, 0)):
        ep = lower_epilogue(c, [Ew("mul", s, Tags(62, 0))], D)
        st, info = capi.classify_ep_status(d, ep)
        assert st == capi.QG_OK and info.supported == 1, info.reason
        got = capi.run_ep(d, ep, np.zeros(M * N, dtype=np.int64), A, B, E)
        exp = oracle.eltwise(ep, c, C, [E[0].astype(np.int64)])
        assert np.array_equal(got, exp), str(D)
        if D.intBits == 62:
            assert (np.abs(exp) >= 1 << 59).any()
        else:
            assert ((exp == D.raw_max) | (exp == D.raw_min)).mean() > 0.05 and (np.abs(exp) < 1 << 49).mean() > 0.05
