"""GPU parity of the piecewise-polynomial activation stage (QG_EW_APPROX, the reference's ANUS::Qapprox) through the C-ABI, all
bit-exact:
  * every golden record of the reference (tests/golden/ref_approx_0) through a K = 1 GEMM whose result IS the record's inputs, on
    the MFMA plan and under QG_OPT_FORCE_TREE;
  * all 65 536 values of a 16-bit C in one 256 x 256 call against a table built by the restatement (tests/approx_ref.py);
  * real GEMMs with chains around the stage: oracle GEMM, oracle.eltwise for the plain stages, the restatement for the stage;
  * the uniform and the general form of the pass on a table both can run (QG_OPT_APPROX_GENERAL, and a result-neutral change of the
    table); a one-segment degree-2 table against the equivalent plain
    four-stage chain; the 64-bit path, ldc > M, the resident-data API with the BitStream export of D, a C++ program on ThenApprox.
The restatement is evaluated once per distinct input value."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import approx_ref as R
from qublas_amd import capi
from qublas_amd.desc import Approx, Ew, Qu, RND, SAT, TRN, WRP, Tags, ew_result, lower, lower_epilogue, lower_epilogue_x

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CASES = R.cases()
BY_NAME = {j["name"]: R.case_table(j) for j in CASES}
ONE = Qu(1, 0, False)


def host_array(vals, q: Qu):
    return np.asarray(vals, dtype=np.int64).astype(np.int32 if q.storage_bits <= 32 else np.int64)


def run_epx(d, ep, tabs, A, B, E, dq: Qu, flags=0, ldc=0, fill=0):
    out = np.full((ldc or d.M) * d.N, fill, dtype=np.int32 if dq.storage_bits <= 32 else np.int64)
    return capi.run_epx(d, ep, tabs, out, A, B, E, flags=flags, ldc=ldc)


def expected(oracle, c: Qu, stages, dq: Qu, x, E):
    """the chain on raw values x (format c): oracle.eltwise for each plain stage (with the assignment that follows it), the
    restatement for an Approx stage and a convert-only oracle.eltwise for its assignment"""
    x = np.asarray(x, dtype=np.int64)
    f = c
    for k, st in enumerate(stages):
        last = k + 1 == len(stages)
        if isinstance(st, Approx):
            x = R.approx(x, f, list(st.segments))
            nxt = dq if last else (st.into or f)
            if nxt != f:
                x = oracle.eltwise(lower_epilogue(f, [], nxt), f, x, [])
        else:
            nxt = dq if last else (st.into or ew_result(f, st))
            x = oracle.eltwise(lower_epilogue(f, [st], nxt), f, x, [E[k]])
        f = nxt
    return x


# ---------------------------------------------------------------- golden records through the identity GEMM
@pytest.mark.parametrize("j", CASES, ids=lambda j: j["name"])
def test_golden_records_through_identity_gemm(j):
    fx, segs = R.case_table(j)
    n = len(j["X"])
    d = lower(fx, ONE, fx, n, 1, 1, mul_args=fx)
    ep, tabs = lower_epilogue_x(fx, [Approx(segs)], fx)
    st, info = capi.classify_epx(d, ep, tabs)
    assert st == capi.QG_OK, info.reason
    A, B = host_array(j["X"], fx), host_array([1], ONE)
    want = np.asarray(j["Y"], dtype=np.int64)
    got = run_epx(d, ep, tabs, A, B, [None], fx)
    assert np.array_equal(got.astype(np.int64), want), (j["name"], capi.KERNEL_NAMES[info.kernel])
    tree = run_epx(d, ep, tabs, A, B, [None], fx, flags=capi.OPT_FORCE_TREE)
    assert np.array_equal(tree.astype(np.int64), want), j["name"]
    # QG_OPT_FUSED_EPILOGUE does not move the stage into a GEMM kernel
    assert np.array_equal(run_epx(d, ep, tabs, A, B, [None], fx, flags=capi.OPT_FUSED_EPILOGUE), got)


def test_golden_plans_cover_both_forms_and_both_widths():
    seen = set()
    for j in CASES:
        fx, segs = R.case_table(j)
        ep, tabs = lower_epilogue_x(fx, [Approx(segs)], fx)
        f = capi.approx_plan_form(lower(fx, ONE, fx, 16, 1, 1, mul_args=fx), ep, tabs)
        seen.add((f.uniform[0], f.bits32))
    assert {(1, 1), (0, 1), (0, 0)} <= seen, seen


# ---------------------------------------------------------------- all 65 536 values of a 16-bit C in one 256 x 256 call
@pytest.mark.parametrize("name", ["probe_four_segments_mixed_modes", "uniform_sigmoid_8x_degree3"])
def test_exhaustive_16_bit_sweep(name):
    """C = A * I (K = 256, the product and every level in x's own format: one term and zeros, nothing rounds or saturates)"""
    fx, segs = BY_NAME[name]
    assert fx.storage_bits == 16
    xs = np.arange(fx.raw_min, fx.raw_max + 1, dtype=np.int64)
    rng = np.random.default_rng(5)
    A = rng.permutation(xs)                       # column-major 256 x 256: element (i, k) at i + 256 k
    eye = np.eye(256, dtype=np.int32).reshape(-1)
    d = lower(fx, ONE, fx, 256, 256, 256, mul_args=fx)
    ep, tabs = lower_epilogue_x(fx, [Approx(segs)], fx)
    got = run_epx(d, ep, tabs, A.astype(np.int32), eye, [None], fx)
    table = R.approx(xs, fx, segs)
    assert np.array_equal(got.astype(np.int64), table[A - fx.raw_min])
    assert len(np.unique(got)) > 100


# ---------------------------------------------------------------- real GEMMs with chains around the stage
E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
E43 = Qu(4, 3)
C158, C238, B106, S34 = Qu(15, 8), Qu(23, 8), Qu(10, 6), Qu(3, 4)
X312 = BY_NAME["uniform_sigmoid_8x_degree3"][0]
SIGMOID = BY_NAME["uniform_sigmoid_8x_degree3"][1]
FA = Qu(4, 10, True, RND.CONV, SAT.TCPL)
FB = Qu(3, 9, True, TRN.TCPL, SAT.ZERO)
FC = Qu(2, 8, True, RND.ZERO, WRP.TCPL)
FD = Qu(5, 6, True, TRN.SMGN, SAT.SMGN)


def wide_table(x: Qu):
    """a general table on the GEMM result's own (wide) format: breakpoints spread over its range, mixed level formats"""
    top = 2.0 ** x.intBits
    return [(-top / 4 + 0.3, [(-1234, FA)]),
            (-0.7, [(700, FB), (-300, FC), (515, FA)]),
            (top / 8, [(-77, FD), (9000, FA), (-2047, FB), (333, FC)]),
            (math.inf, [(-2047, FD), (5, FC)])]


def chains(cq: Qu):
    return {
        "scale_bias_act": ([Ew("mul", S34, Tags(24, 8), scalar=True, into=Qu(24, 8)), Ew("add", B106, into=X312), Approx(SIGMOID)],
                           Qu(1, 10, True, RND.CONV, SAT.TCPL)),
        "act_mul_tensor": ([Approx(wide_table(cq)), Ew("mul", S34)], Qu(12, 6, True, RND.ZERO, SAT.TCPL)),
        "act_alone_narrow": ([Approx(wide_table(cq))], Qu(4, 3, True, RND.INF, SAT.SMGN)),
    }


def _operands(oracle, stages, n, seed0=170):
    Eo, Eh = [], []
    for k, st in enumerate(stages):
        if isinstance(st, Approx):
            Eo.append(None)
            Eh.append(None)
            continue
        h = oracle.fill(st.e, 1 if st.scalar else n, seed0 + k, 0)
        Eh.append(h)
        Eo.append(h.astype(np.int64))
    return Eo, Eh


@pytest.mark.parametrize("chain", ["scale_bias_act", "act_mul_tensor", "act_alone_narrow"])
@pytest.mark.parametrize("cfg", ["limb", "i8", "tree", "limb_wideC"])
def test_gemm_plus_chain_vs_oracle(oracle, cfg, chain):
    if cfg.startswith("limb"):      # 3x3 int8 limbs
        cq = C238 if cfg == "limb_wideC" else C158
        ea, M, N, K, kw, kern = E88, 200, 136, 192, dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)]), "mfma_i8_limb"
    elif cfg == "i8":               # single limb
        ea, cq, M, N, K, kw, kern = E43, C158, 130, 260, 128, dict(mul_args=Tags(9, 6), add_args=[Qu(21, 6)]), "mfma_i8"
    else:                           # default tags: exact tree kernel
        ea, cq, M, N, K, kw, kern = E88, E88, 96, 80, 128, dict(), "tree_i32"
    stages, dq = chains(cq)[chain]
    d = lower(ea, ea, cq, M, N, K, **kw)
    ep, tabs = lower_epilogue_x(cq, stages, dq)
    st, info = capi.classify_epx(d, ep, tabs)
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == kern, info.reason
    dist = 1 if cfg != "tree" else 0
    A, B = oracle.fill(ea, M * K, 1, dist), oracle.fill(ea, K * N, 2, dist)
    Eo, Eh = _operands(oracle, stages, M * N)
    got = run_epx(d, ep, tabs, A, B, Eh, dq)
    Cx = oracle.gemm(d, A, B, cq, nthreads=8).astype(np.int64)
    assert np.array_equal(got.astype(np.int64), expected(oracle, cq, stages, dq, Cx, Eo))
    assert len(np.unique(got)) > 8   # the comparison is not hidden by saturation
    if cfg != "tree":
        assert np.array_equal(run_epx(d, ep, tabs, A, B, Eh, dq, flags=capi.OPT_FORCE_TREE), got)


# ---------------------------------------------------------------- uniform form = general form
def test_uniform_and_general_form_agree(oracle):
    """A top coefficient 0 in front of a segment changes nothing (Qmul(x, 0) = 0 and Qadd(a, 0) = a in a's own format) but the
    segment's length: the table then takes the general form.  Same bytes, and both equal the restatement."""
    M, N = 333, 77                                  # 25 641 elements: more than one block, not a multiple of 16
    zero_top = [(bp, list(c) + ([(0, c[-1][1])] if s == 2 else [])) for s, (bp, c) in enumerate(SIGMOID)]
    rng = np.random.default_rng(11)
    xs = rng.integers(X312.raw_min, X312.raw_max + 1, M * N)
    d = lower(X312, ONE, X312, M * N, 1, 1, mul_args=X312)
    outs = []
    with capi.Context() as ctx:
        for segs, uniform in ((SIGMOID, 1), (zero_top, 0)):
            ep, tabs = lower_epilogue_x(X312, [Approx(segs)], X312)
            plan = capi.Plan(ctx, d, epilogue=ep, approx=tabs)
            assert plan.approx_uniform() == uniform and not plan.fuses_epilogue()
            plan.close()
            outs.append(run_epx(d, ep, tabs, xs.astype(np.int32), host_array([1], ONE), [None], X312))
    assert np.array_equal(outs[0], outs[1])
    assert np.array_equal(outs[0].astype(np.int64), R.approx(xs, X312, SIGMOID))


@pytest.mark.parametrize("fx", [X312, Qu(15, 12)], ids=["32-bit", "64-bit"])
def test_general_form_flag_on_a_uniform_table(fx):
    """QG_OPT_APPROX_GENERAL sends a uniform table through the general form of the pass (the product library's result-identical
    form choice, like QG_OPT_GENERIC_LAYOUT): same bytes as the uniform form, both the restatement's; in 32- and 64-bit arithmetic"""
    n = 25641                                       # more than one block, not a multiple of 16
    xs = np.random.default_rng(11).integers(-(1 << 15), 1 << 15, n)   # +-8: every segment of the logistic fit
    d = lower(fx, ONE, fx, n, 1, 1, mul_args=fx)
    ep, tabs = lower_epilogue_x(fx, [Approx(SIGMOID)], fx)
    form = capi.approx_plan_form(d, ep, tabs)
    assert form.uniform[0] == 1 and form.bits32 == (1 if fx == X312 else 0)
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, flags=capi.OPT_APPROX_GENERAL, epilogue=ep, approx=tabs)
        assert plan.approx_uniform() == 1           # the table's form; the flag only changes which form runs
        plan.close()
    A, B = host_array(xs, fx), host_array([1], ONE)
    uni = run_epx(d, ep, tabs, A, B, [None], fx)
    gen = run_epx(d, ep, tabs, A, B, [None], fx, flags=capi.OPT_APPROX_GENERAL)
    assert np.array_equal(uni, gen)
    assert np.array_equal(uni.astype(np.int64), R.approx(xs, fx, SIGMOID)) and len(np.unique(uni)) > 100


# ---------------------------------------------------------------- one segment of degree 2 = the plain four-stage chain
def test_one_segment_table_equals_the_plain_chain(oracle):
    """a0 + x (a1 + x a2) with x as a tensor operand of the existing stages: x0 = a2 (scalar C of a K = 1 GEMM),
    Qmul<f1>(x0, X), Qadd<f1>(a1, .), Qmul<f0>(., X), Qadd<f0>(a0, .), converted into x's type"""
    fx, segs = BY_NAME["one_segment_degree2"]
    (a0, f0), (a1, f1), (a2, f2) = segs[0][1]
    M, N = 250, 41
    n = M * N
    xs = np.random.default_rng(3).integers(fx.raw_min, fx.raw_max + 1, n)
    X = host_array(xs, fx)
    d = lower(fx, ONE, fx, n, 1, 1, mul_args=fx)
    ep, tabs = lower_epilogue_x(fx, [Approx(segs)], fx)
    got = run_epx(d, ep, tabs, X, host_array([1], ONE), [None], fx)
    # the plain chain: C = a2 everywhere (format f2)
    d2 = lower(f2, ONE, f2, n, 1, 1, mul_args=f2)
    stages = [Ew("mul", fx, f1, x_first=False), Ew("add", f1, f1, x_first=False, scalar=True),
              Ew("mul", fx, f0, x_first=False), Ew("add", f0, f0, x_first=False, scalar=True)]
    ep2 = lower_epilogue(f2, stages, fx)
    out2 = np.zeros(n, dtype=np.int32)
    capi.run_ep(d2, ep2, out2, host_array([a2] * n, f2), host_array([1], ONE), [X, host_array([a1], f1), X, host_array([a0], f0)])
    assert np.array_equal(got, out2)
    assert np.array_equal(got.astype(np.int64), R.approx(xs, fx, segs)) and len(np.unique(got)) > 50


# ---------------------------------------------------------------- remaining paths
def test_64_bit_path_with_column_padding():
    """x of 40 value bits (int64 containers, 64-bit arithmetic), ldc > M: the padding between the columns is kept"""
    fx, segs = BY_NAME["x_of_40_value_bits"]
    M, N, ldc = 45, 7, 50
    rng = np.random.default_rng(9)
    xs = np.concatenate([rng.integers(fx.raw_min, fx.raw_max + 1, M * N - 128), rng.integers(-(1 << 24), 1 << 24, 64), rng.integers(-(1 << 36), 1 << 36, 64)])
    # C = A * I with K = N: column j of C is column j of A (one term and zeros: nothing rounds or saturates)
    d = lower(fx, ONE, fx, M, N, N, mul_args=fx)
    ep, tabs = lower_epilogue_x(fx, [Approx(segs)], fx)
    assert capi.approx_plan_form(d, ep, tabs).bits32 == 0
    assert {R.select(int(v), fx, segs) for v in xs} == {0, 1, 2}
    got = run_epx(d, ep, tabs, xs.astype(np.int64), np.eye(N, dtype=np.int32).reshape(-1), [None], fx, ldc=ldc, fill=-777)
    o2 = got.reshape(N, ldc)
    assert np.array_equal(o2[:, :M].reshape(-1), R.approx(xs, fx, segs)) and (o2[:, M:] == -777).all()


def test_resident_api_and_bitstream_of_d(oracle):
    """plan_create_epx / execute_ep on resident buffers; the stage has no packed operand; BitStream export of D"""
    cq = C158
    stages, dq = chains(cq)["scale_bias_act"]
    M = N = K = 256
    d = lower(E88, E88, cq, M, N, K, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
    ep, tabs = lower_epilogue_x(cq, stages, dq)
    A, B = oracle.fill(E88, M * K, 1, 1), oracle.fill(E88, K * N, 2, 1)
    Eo, Eh = _operands(oracle, stages, M * N)
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, epilogue=ep, approx=tabs)
        assert plan.packed_e_bytes(2) == 0 and plan.packed_e_bytes(1) > 0 and plan.approx_uniform() == 1 and not plan.fuses_epilogue()
        dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
        ctx.h2d(dA, A); ctx.h2d(dB, B)
        pA, pB, pD = (ctx.alloc(int(plan.info.packed_bytes[i])) for i in range(3))
        plan.pack(capi.OPERAND_A, dA, pA); plan.pack(capi.OPERAND_B, dB, pB)
        dE = ctx.alloc(Eh[1].nbytes); ctx.h2d(dE, Eh[1])
        pE = ctx.alloc(plan.packed_e_bytes(1)); plan.pack_e(1, dE, pE)
        args = plan.ep_args(packed=[0, pE, 0], scalars=[int(Eo[0][0]), 0, 0])
        with pytest.raises(capi.QgemulError):
            plan.execute(pD, pA, pB)
        plan.execute_ep(pD, pA, pB, args)
        out = np.zeros(M * N, dtype=np.int32)
        dD = ctx.alloc(out.nbytes)
        plan.unpack_c(pD, dD)
        ctx.d2h(out, dD)
        bits = np.zeros(plan.bitstream_bytes(capi.BITS_ASCII), dtype=np.uint8)
        dS = ctx.alloc(bits.nbytes)
        plan.export_bitstream(pD, dS, 0, 0, capi.BITS_ASCII)
        ctx.d2h(bits, dS)
        assert plan.time_execute_ep(pD, pA, pB, args, 1, 2) > 0
        # the chain alone on a C tensor that already exists (here the oracle's): the same D
        Cx = oracle.gemm(d, A, B, cq, nthreads=8)
        dC = ctx.alloc(Cx.nbytes); ctx.h2d(dC, Cx)
        assert plan.packed_c_bytes() > 0 and plan.packed_e_bytes(-1) == 0
        pC = ctx.alloc(plan.packed_c_bytes()); plan.pack_c(dC, pC)
        pD2 = ctx.alloc(int(plan.info.packed_bytes[2]))
        plan.apply_epilogue(pD2, pC, args)
        out2 = np.zeros(M * N, dtype=np.int32)
        plan.unpack_c(pD2, dD)
        ctx.d2h(out2, dD)
        assert plan.time_apply_epilogue(pD2, pC, args, 1, 2) > 0
        plan.close()
    exp = expected(oracle, cq, stages, dq, Cx.astype(np.int64), Eo)
    assert np.array_equal(out.astype(np.int64), exp) and np.array_equal(out2, out)
    assert bits.tobytes() == oracle.bitstream(dq, exp)


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_then_approx_on_gpu(tmp_path, oracle):
    """Qgemul<…, QgemulResult<CT>>(D, A, B, ThenMul<…>(s), ThenAdd<…>(Bias), ThenApprox<…>()) through include/QuBLAS_amd.h"""
    exe = tmp_path / "amd_header_approx_run"
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++23", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "binding", "amd_header_approx_run.cpp"), "-o", str(exe), "-L" + lib, "-lqugemm",
                           "-Wl,-rpath," + lib])
    r = json.loads(subprocess.check_output([str(exe)], text=True).strip().splitlines()[0])
    assert "error" not in r, r
    M, N, K = r["M"], r["N"], r["K"]
    cq = C158
    stages, dq = chains(cq)["scale_bias_act"]
    d = lower(E88, E88, cq, M, N, K, mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
    i = np.arange(M * K, dtype=np.uint64)
    A = ((i * np.uint64(2654435761)) % np.uint64(128)).astype(np.int64) - 64
    i = np.arange(K * N, dtype=np.uint64)
    B = ((i * np.uint64(40503) + np.uint64(7)) % np.uint64(128)).astype(np.int64) - 64
    i = np.arange(M * N, dtype=np.uint64)
    bias = ((i * np.uint64(97)) % np.uint64(512)).astype(np.int64) - 256
    Cx = oracle.gemm(d, A.astype(np.int32), B.astype(np.int32), cq).astype(np.int64)
    exp = expected(oracle, cq, stages, dq, Cx, [np.array([13]), bias, None])
    assert r["D"] == exp.tolist() and len(set(r["D"])) > 20
