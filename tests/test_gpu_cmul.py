"""GPU parity of complex chains that hold a complex x complex multiplication (include/qgemul.h, QG_EW_CMUL), through the C-ABI:
  * every golden vector of the reference's lazy tensor Qmul on complex tensors (tests/golden/ref_cplx_cmul_0), fed through a K = 1
    complex GEMM whose result IS the fixture's X tensor;
  * complex GEMMs of both packed-C producers (the 32-bit tree kernel, the stacked MFMA linear class) at sizes that end in the pass
    kernel's tail, its body, or both, plus chains of both arithmetic widths, against oracle GEMM + tests/cmul_ref.py;
  * all 65 536 (x, e) pairs of two complex formats with 4-bit parts;
  * the resident entry points, the chain alone on a packed C, the BitStream of D, a padded ldc, and the one-shot cache.
The GEMM is not what is tested: K stays at 32 / 64."""
import numpy as np
import pytest

import cmul_ref as R
from qublas_amd import capi
from qublas_amd.desc import (BasicComplexMul, EwC, Qcomplex, Qu, RND, SAT, TRN, WRP, Tags, TFComplexMul, host_layout, lower,
                             lower_epilogue_cplx_x)

pytestmark = pytest.mark.gpu

CASES = R.cases()
ONE = Qu(1, 0, False)
CONE = Qcomplex(ONE, ONE)


def host_elems(oracle, e, re, im=None):
    out = np.zeros(len(re), dtype=oracle.host_dtype(e))
    if isinstance(e, Qcomplex):
        out["re"], out["im"] = re, im
    else:
        out[:] = re
    return out


def parts(h):
    return h["re"].astype(np.int64), h["im"].astype(np.int64)


def run_epcx(oracle, d, epc, cx, A, B, E, dq, flags=0, ldc=0):
    out = np.zeros((ldc or d.M) * d.N, dtype=oracle.host_dtype(dq))
    return capi.run_epcx(d, epc, cx, out, A, B, E, flags=flags, ldc=ldc)


def identity_gemm(c, n, N=1):
    """C = X * (1 + 0i) with K = 1: re = a*1 - b*0 and im = a*0 + b*1 in C's own part formats reproduce X exactly"""
    return lower(c, CONE, c, n, N, 1, mul_args=BasicComplexMul(acT=c.real, bdT=c.imag, adT=c.real, bcT=c.imag, acbdT=c.real, adbcT=c.imag))


@pytest.mark.parametrize("j", CASES, ids=lambda j: j["name"])
def test_golden_vectors_through_identity_gemm(oracle, j):
    epc, cx, c, dq = R.case_chain(j)
    d = identity_gemm(c, j["n"])
    A = host_elems(oracle, c, j["Xre"], j["Xim"])
    B = host_elems(oracle, CONE, [1], [0])
    Eh = []
    for s in j["stages"]:
        e = [Qu.from_tuple(t) for t in s["e"]]
        Eh.append(host_elems(oracle, Qcomplex(e[0], e[1]) if s["e_complex"] else e[0], s["Ere"], s["Eim"]))
    got = run_epcx(oracle, d, epc, cx, A, B, Eh, dq)
    assert np.array_equal(got["re"].astype(np.int64), np.asarray(j["Dre"], dtype=np.int64)), j["name"]
    assert np.array_equal(got["im"].astype(np.int64), np.asarray(j["Dim"], dtype=np.int64)), j["name"]


# ---- behind real GEMMs ----
R63 = Qu(6, 3, True, RND.POS_INF, SAT.TCPL)
R6N3 = Qu(6, -3, True, RND.POS_INF, SAT.TCPL)
C5 = Qcomplex(R63, R6N3)
WIDE4 = Qcomplex(Qu(18, 6, True, RND.POS_INF), Qu(18, 6, True, RND.POS_INF))      # 25 storage bits: 4-byte packed C
WIDE8 = Qcomplex(Qu(30, 6, True, RND.POS_INF), Qu(30, 6, True, RND.POS_INF))      # 37 storage bits: 8-byte packed C
BL = BasicComplexMul(acT=Qu(14, 6), bdT=Qu(14, -6), adT=Qu(14, 0), bcT=Qu(14, 0), acbdT=Qu(15, 6), adbcT=Qu(15, 0))
LIN = dict(mul_args=BL, add_args=[Qcomplex(Qu(30, 6), Qu(30, 0))])
GEMMS = {
    # name: (C type, M, N, K, lowering keywords, kernel).  The pass kernel gives a lane 8 consecutive elements of each half of the
    # row-major packed C [2][M][N]: 1 and 15 elements are tail only, 561 is body + tail, 3072 body only
    "tree_1x1": (C5, 1, 1, 32, dict(mul_args=TFComplexMul()), "tree_cplx_i32"),
    "tree_3x5": (C5, 3, 5, 32, dict(mul_args=TFComplexMul()), "tree_cplx_i32"),
    "tree_33x17": (C5, 33, 17, 32, dict(mul_args=TFComplexMul()), "tree_cplx_i32"),
    "tree_64x48": (C5, 64, 48, 32, dict(mul_args=TFComplexMul()), "tree_cplx_i32"),
    "linear4_33x17": (WIDE4, 33, 17, 64, LIN, "mfma_cplx"),
    "linear4_129x130": (WIDE4, 129, 130, 64, LIN, "mfma_cplx"),
    "linear8_33x17": (WIDE8, 33, 17, 64, LIN, "mfma_cplx"),
    "linear8_129x130": (WIDE8, 129, 130, 64, LIN, "mfma_cplx"),
}
E1 = Qcomplex(Qu(3, 4), Qu(2, 5))                                 # 1-byte containers
E2 = Qcomplex(Qu(5, 6), Qu(7, 4, False))                          # 2-byte
E4 = Qcomplex(Qu(14, 8), Qu(14, 8))                               # 4-byte
E8 = Qcomplex(Qu(24, 12), Qu(20, 12))                             # 8-byte
D1 = Qcomplex(Qu(4, 3, True, RND.CONV, SAT.TCPL), Qu(5, 2, True, TRN.SMGN, WRP.TCPL))
D2 = Qcomplex(Qu(9, 5, True, RND.INF, SAT.SMGN), Qu(11, 3, True, RND.ZERO, SAT.ZERO))
D4 = Qcomplex(Qu(16, 8), Qu(20, 2, True, RND.NEG_INF))
D8 = Qcomplex(Qu(34, 10), Qu(30, 12))
NARROW = Qcomplex(Qu(6, 4, True, RND.POS_INF), Qu(6, 2))
TB = BasicComplexMul(acT=Tags(fracBits=3, QuMode=RND.CONV), bdT=Tags(intBits=5, OfMode=WRP.TCPL), adbcT=Tags(QuMode=RND.ZERO, fracBits=2))
TT = TFComplexMul(abT=Tags(intBits=8), abcT=Tags(fracBits=3, QuMode=RND.INF), badT=Tags(OfMode=SAT.ZERO), BCT=Tags(fracBits=2, QuMode=TRN.SMGN))
CHAINS = {
    # Basic / TF, both orders, tensor / scalar e, e and d containers of 1, 2, 4, 8 bytes, stages before and after the CMUL
    "basic_tensor_e1_d1": ([EwC("mul", E1, tags=TB, into=NARROW)], D1),
    "tf_efirst_tensor_e2_d2": ([EwC("mul", E2, tags=TT, x_first=False)], D2),
    "basic_scalar_efirst_d4": ([EwC("mul", E2, tags=TB, x_first=False, scalar=True)], D4),
    "tf_scalar_d8": ([EwC("mul", E1, tags=TT, scalar=True)], D8),
    "cadd_cmul_e4_real_scale": ([EwC("add", E1, into=NARROW), EwC("mul", E4, tags=BasicComplexMul(loose=Tags(FullPrec=True)), into=D4),
                                 EwC("mul", Qu(2, 2), scalar=True)], D4),
    "tf_tensor_e8_d8": ([EwC("mul", E8, tags=TFComplexMul(abcT=Tags(FullPrec=True), cdbT=Tags(FullPrec=True), badT=Tags(FullPrec=True)))], D8),
    "real_mul_cmul_e1_cadd_scalar": ([EwC("mul", Qu(2, 2), into=NARROW), EwC("mul", E1, tags=TT, x_first=False, into=NARROW),
                                      EwC("add", E1, scalar=True)], D2),
}
_GEMM_CACHE = {}


def gemm_case(oracle, name):
    """(descriptor, A, B, the oracle's C parts): computed once per GEMM"""
    if name not in _GEMM_CACHE:
        ec, M, N, K, kw, _ = GEMMS[name]
        d = lower(C5, C5, ec, M, N, K, **kw)
        A, B = oracle.fill(C5, M * K, 11, 0), oracle.fill(C5, K * N, 12, 0)
        _GEMM_CACHE[name] = (d, A, B, parts(oracle.gemm(d, A, B, ec, nthreads=8)))
    return _GEMM_CACHE[name]


def operands(oracle, stages, n, seed0=130):
    """host arrays for the call and the per-part value lists for the restatement"""
    Eh, Ere, Eim = [], [], []
    for k, st in enumerate(stages):
        h = oracle.fill(st.e, 1 if st.scalar else n, seed0 + k, 0)
        Eh.append(h)
        if isinstance(st.e, Qcomplex):
            re, im = parts(h)
        else:
            re = h.astype(np.int64)
            im = re if st.op == "mul" else np.zeros(1, dtype=np.int64)
        Ere.append(re)
        Eim.append(im)
    return Eh, Ere, Eim


# (an 8-byte operand part times an 8-byte C part is a 74-bit product: refused, tests/test_cmul_plan.py)
PAIRS = [(g, c) for g in sorted(GEMMS) for c in sorted(CHAINS) if not (g.startswith("linear8") and c == "tf_tensor_e8_d8")]


@pytest.mark.parametrize("gemm,chain", PAIRS)
def test_complex_gemm_plus_chain_vs_restatement(oracle, gemm, chain):
    ec, M, N, K, kw, kern = GEMMS[gemm]
    stages, dq = CHAINS[chain]
    d, A, B, (cre, cim) = gemm_case(oracle, gemm)
    epc, cx = lower_epilogue_cplx_x(ec, stages, dq)
    st, info = capi.classify_epcx(d, epc, cx)
    assert st == capi.QG_OK, info.reason
    assert capi.KERNEL_NAMES[info.kernel] == kern
    Eh, Ere, Eim = operands(oracle, stages, M * N)
    got = run_epcx(oracle, d, epc, cx, A, B, Eh, dq)
    exp_re, exp_im = R.chain(epc, cx, ec, cre, cim, Ere, Eim)
    assert np.array_equal(got["re"].astype(np.int64), exp_re)
    assert np.array_equal(got["im"].astype(np.int64), exp_im)
    if gemm.startswith("tree") and M * N >= 500:   # (the linear GEMMs' 25- / 37-bit C saturates the narrow destinations by design)
        assert len(np.unique(got["re"])) > 8 and len(np.unique(got["im"])) > 8   # not hidden by saturation


def test_both_arithmetic_widths_and_all_containers_ran():
    """what the cases above cover, from the planner (pure host code)"""
    widths = {}
    for gemm, (ec, M, N, K, kw, _) in GEMMS.items():
        d = lower(C5, C5, ec, M, N, K, **kw)
        for chain, (stages, dq) in CHAINS.items():
            if (gemm, chain) not in PAIRS:
                continue
            epc, cx = lower_epilogue_cplx_x(ec, stages, dq)
            st, form = capi.cmul_plan_form(d, epc, cx)
            assert st == capi.QG_OK and form.has_cmul == 1
            widths.setdefault(gemm.split("_")[0], set()).add(form.bits32)
    assert widths["tree"] == {0, 1} and widths["linear4"] == {0, 1} and widths["linear8"] == {0}
    cont = lambda q: max(1 << max(0, (f.storage_bits - 1).bit_length() - 3) for f in (q.real, q.imag))
    assert [cont(e) for e in (E1, E2, E4, E8)] == [1, 2, 4, 8] and [cont(e) for e in (D1, D2, D4, D8)] == [1, 2, 4, 8]


# ---- every pair of two complex formats with 4-bit parts ----
X4 = Qcomplex(Qu(1, 2), Qu(2, 1))                                 # 16 raw values per part
Y4 = Qcomplex(Qu(2, 1), Qu(0, 3))
SWEEPS = {
    "basic_saturating": (BasicComplexMul(acT=Qu(2, 2, True, RND.POS_INF, SAT.TCPL), bdT=Qu(2, 1, True, RND.CONV, SAT.SMGN), adT=Qu(1, 3, True, TRN.SMGN, SAT.ZERO),
                                         bcT=Qu(2, 2, True, RND.ZERO, SAT.TCPL), acbdT=Qu(2, 1, True, RND.INF, SAT.SMGN), adbcT=Qu(2, 2, True, RND.NEG_INF, SAT.TCPL)),
                         Qcomplex(Qu(2, 1), Qu(2, 2))),
    "basic_wrapping": (BasicComplexMul(loose=Tags(intBits=2, fracBits=2, QuMode=RND.CONV, OfMode=WRP.TCPL)), Qcomplex(Qu(2, 2), Qu(2, 2))),
    "tf_saturating": (TFComplexMul(abT=Qu(2, 2, True, TRN.TCPL, SAT.SMGN), cdT=Qu(2, 2, True, TRN.TCPL, SAT.TCPL), abcT=Qu(2, 2, True, RND.POS_INF, SAT.ZERO),
                                   badT=Qu(3, 1, True, RND.CONV, SAT.TCPL), cdbT=Qu(2, 2, True, RND.INF, SAT.SMGN), ABT=Qu(2, 1, True, RND.ZERO, SAT.TCPL),
                                   BCT=Qu(3, 1, True, TRN.SMGN, SAT.SMGN)), Qcomplex(Qu(2, 1), Qu(3, 1))),
    "tf_wrapping": (TFComplexMul(loose=Tags(intBits=2, fracBits=2, QuMode=RND.NEG_INF, OfMode=WRP.TCPL)), Qcomplex(Qu(2, 2), Qu(2, 2))),
}


def all_pairs(oracle):
    """X[i, j] = x_i, E[i, j] = e_j over all 256 values of each complex format; column-major 256 x 256"""
    v = np.arange(-8, 8, dtype=np.int64)
    xa, xb = np.repeat(v, 16), np.tile(v, 16)                    # the 256 complex values (re, im)
    i, j = np.tile(np.arange(256), 256), np.repeat(np.arange(256), 256)   # element i + 256 j
    return (xa[i], xb[i]), (xa[j], xb[j])


@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_exhaustive_pairs_of_4bit_part_formats(oracle, name):
    """the chain alone (qgemul_pack_c + qgemul_apply_epilogue) on a 256 x 256 tensor that holds all 65 536 (x, e) pairs"""
    tags, dq = SWEEPS[name]
    (xre, xim), (ere, eim) = all_pairs(oracle)
    epc, cx = lower_epilogue_cplx_x(X4, [EwC("mul", Y4, tags=tags)], dq)
    d = lower(X4, X4, X4, 256, 256, 8, mul_args=TFComplexMul())
    exp_re, exp_im = R.chain(epc, cx, X4, xre, xim, [ere], [eim])
    out = apply_alone(oracle, d, epc, cx, X4, dq, host_elems(oracle, X4, xre, xim), [host_elems(oracle, Y4, ere, eim)])
    assert np.array_equal(out["re"].astype(np.int64), exp_re) and np.array_equal(out["im"].astype(np.int64), exp_im)
    assert len(np.unique(exp_re)) > 8 and len(np.unique(exp_im)) > 8


def apply_alone(oracle, d, epc, cx, c, dq, Ch, Eh, scalars=(), scalars_im=(), bits=None):
    """plan_create_epcx / pack_c / pack_e / apply_epilogue / unpack_c on device-resident tensors; bits: also the ASCII BitStream of D"""
    n = d.M * d.N
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, epilogue=epc, cmul=cx)
        assert not plan.fuses_epilogue()
        dC, pC = ctx.alloc(Ch.nbytes), ctx.alloc(plan.packed_c_bytes())
        ctx.h2d(dC, Ch)
        plan.pack_c(dC, pC)
        packed = []
        for k, h in enumerate(Eh):
            if h is None:
                assert plan.packed_e_bytes(k) == 0
                packed.append(0)
                continue
            nb = plan.packed_e_bytes(k)
            assert nb > 0
            dE, pE = ctx.alloc(h.nbytes), ctx.alloc(nb)
            ctx.h2d(dE, h)
            plan.pack_e(k, dE, pE)
            packed.append(pE)
        pD = ctx.alloc(int(plan.info.packed_bytes[2]))
        plan.apply_epilogue(pD, pC, plan.ep_args(packed=packed, scalars=scalars, scalars_im=scalars_im))
        size, _, _ = host_layout(dq)
        assert plan.info.host_elem_bytes[2] == size
        dD = ctx.alloc(n * size)
        plan.unpack_c(pD, dD)
        out = np.zeros(n, dtype=oracle.host_dtype(dq))
        ctx.d2h(out, dD)
        if bits is not None:
            nb = plan.bitstream_bytes(capi.BITS_ASCII)
            dev = ctx.alloc(nb)
            plan.export_bitstream(pD, dev, 0, 0, capi.BITS_ASCII)
            s = np.zeros(nb, dtype=np.uint8)
            ctx.d2h(s, dev)
            bits.append(s.tobytes())
        plan.close()
    return out


def test_chain_alone_on_a_packed_c_and_the_bitstream_of_d(oracle):
    """a tensor that no GEMM made, a tensor stage and a scalar stage, D exported as the reference's BitStream"""
    ec, M, N, K, kw, _ = GEMMS["tree_33x17"]
    stages = [EwC("mul", E2, tags=TT, into=NARROW), EwC("mul", E1, tags=TB, x_first=False, scalar=True)]
    epc, cx = lower_epilogue_cplx_x(ec, stages, D2)
    d = lower(C5, C5, ec, M, N, K, **kw)
    Ch = oracle.fill(ec, M * N, 21, 0)
    Eh, Ere, Eim = operands(oracle, stages, M * N, seed0=22)
    exp_re, exp_im = R.chain(epc, cx, ec, *parts(Ch), Ere, Eim)
    bits = []
    out = apply_alone(oracle, d, epc, cx, ec, D2, Ch, [Eh[0], None], scalars=[0, int(Ere[1][0])], scalars_im=[0, int(Eim[1][0])], bits=bits)
    assert np.array_equal(out["re"].astype(np.int64), exp_re) and np.array_equal(out["im"].astype(np.int64), exp_im)
    assert bits[0] == oracle.bitstream_cplx(D2, exp_re, exp_im, 0, 0)


def test_resident_gemm_plus_chain_and_a_padded_ldc(oracle):
    """qgemul_plan_create_epcx / qgemul_pack_e / qgemul_execute_ep / qgemul_unpack_c with ld > M; the one-shot entry with ldc > M"""
    name = "linear4_33x17"
    ec, M, N, K, kw, _ = GEMMS[name]
    stages, dq = CHAINS["cadd_cmul_e4_real_scale"]
    d, A, B, (cre, cim) = gemm_case(oracle, name)
    epc, cx = lower_epilogue_cplx_x(ec, stages, dq)
    Eh, Ere, Eim = operands(oracle, stages, M * N, seed0=40)
    exp_re, exp_im = R.chain(epc, cx, ec, cre, cim, Ere, Eim)
    ld = M + 5
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, epilogue=epc, cmul=cx)
        assert not plan.fuses_epilogue()
        dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
        ctx.h2d(dA, A); ctx.h2d(dB, B)
        pA, pB, pD = (ctx.alloc(int(plan.info.packed_bytes[i])) for i in range(3))
        plan.pack(capi.OPERAND_A, dA, pA); plan.pack(capi.OPERAND_B, dB, pB)
        packed = []
        for k in range(2):
            dE, pE = ctx.alloc(Eh[k].nbytes), ctx.alloc(plan.packed_e_bytes(k))
            ctx.h2d(dE, Eh[k])
            plan.pack_e(k, dE, pE)
            packed.append(pE)
        assert plan.packed_e_bytes(2) == 0
        plan.execute_ep(pD, pA, pB, plan.ep_args(packed=packed + [0], scalars=[0, 0, int(Ere[2][0])], scalars_im=[0, 0, int(Eim[2][0])]))
        out = np.full(ld * N, -1, dtype=oracle.host_dtype(dq))
        dD = ctx.alloc(out.nbytes)
        ctx.h2d(dD, out)
        plan.unpack_c(pD, dD, ld=ld)
        ctx.d2h(out, dD)
        plan.close()
    body = out.reshape(N, ld)
    assert np.array_equal(body[:, :M].reshape(-1)["re"].astype(np.int64), exp_re) and np.array_equal(body[:, :M].reshape(-1)["im"].astype(np.int64), exp_im)
    assert np.all(body[:, M:]["re"] == -1) and np.all(body[:, M:]["im"] == -1)          # the padding is kept
    pad = run_epcx(oracle, d, epc, cx, A, B, Eh, dq, ldc=ld)
    assert np.array_equal(pad.reshape(N, ld)[:, :M], body[:, :M])


def test_one_shot_rebuilds_its_plan_when_only_the_cmul_record_changes(oracle):
    """two chains with byte-identical qgemul_epilogue_cplx (the RE / IM formats are named) that differ in one product's QuMode"""
    name = "tree_33x17"
    ec, M, N, K, kw, _ = GEMMS[name]
    d, A, B, (cre, cim) = gemm_case(oracle, name)
    full = dict(acbdT=Qu(8, 3), adbcT=Qu(8, 3))
    variants = [BasicComplexMul(acT=Tags(fracBits=1, QuMode=q), **full) for q in (TRN.TCPL, RND.POS_INF, TRN.TCPL)]
    lowered = [lower_epilogue_cplx_x(ec, [EwC("mul", E1, tags=t)], D2) for t in variants]
    assert bytes(lowered[0][0]) == bytes(lowered[1][0]) and bytes(lowered[0][1][0]) != bytes(lowered[1][1][0])
    Eh, Ere, Eim = operands(oracle, [EwC("mul", E1)], M * N, seed0=50)
    results = []
    for epc, cx in lowered:
        got = run_epcx(oracle, d, epc, cx, A, B, Eh, D2)
        exp_re, exp_im = R.chain(epc, cx, ec, cre, cim, Ere, Eim)
        assert np.array_equal(got["re"].astype(np.int64), exp_re) and np.array_equal(got["im"].astype(np.int64), exp_im)
        results.append(got.copy())
    assert not np.array_equal(results[0], results[1]) and np.array_equal(results[0], results[2])
