"""GPU parity of Qgemul with one real and one complex operand (QG_CMUL_REAL_A / QG_CMUL_REAL_B, include/qgemul.h), through the C-ABI.
Every comparison is byte for byte against tests/mixed_ref.py — part p of the descriptor as a real Qgemul through the oracle —, which
the CPU tests pin to the reference's own results (tests/golden/ref_mixed_0):
  * every golden record through qgemul_run and through the resident entry points, and under QG_OPT_RUNTIME_MODES, QG_OPT_GENERIC_TREE
    and (linear class) QG_OPT_FORCE_TREE;
  * the mixed tree kernel (k_tree_rc: compact steps and, under QG_OPT_RUNTIME_MODES or with modes the compact steps lack, run-time
    modes) and the general kernel's part-wise branch (QG_OPT_GENERIC_TREE), both operand orders: shapes that cross the 32 x 32 and
    16 x 16 tiles in both directions, K below / at / above one 32-leaf chunk with odd leftovers on several
    levels, 12 and 13 levels, TransposedA; edge-heavy operands (dist 2) at 33 x 17 x 33 and 65 x 40 x 1000;
  * the linear class (one real limb GEMM on the stacked operand + the two-product convert pass): one-, two- and three-limb operands,
    parts whose shifts into C differ, 33 x 17 x 40 and 130 x 70 x 200, TransposedA, and the same descriptors under QG_OPT_FORCE_TREE
    (every other tile form of that GEMM: tests/test_gpu_stacked_tiles.py);
  * QG_OPT_CHECK_RANGE, qgemul_execute_host_c and qgemul_time_execute on mixed plans;
  * 128-bit values (a level format of 70 bits) at 9 x 7 x 37;
  * leading dimensions with poison between the columns, qgemul_pack_f64, qgemul_fill_packed against the oracle's generator, the
    BitStream of one result, qgemul_run from two threads;
  * the standalone header's Qgemul<...>(C, A, B) on (real tensor, complex tensor) and (complex, real): tests/binding/amd_header_mixed_run.cpp.
Strength: in every case not labelled a saturation case at least half of each part's outputs are neither zero nor at a bound of C
(asserted on the checker's output)."""
import functools
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import mixed_ref as R
from stacked_cases import LINEAR   # (the linear-class elements and tags: shared with tests/test_gpu_stacked_tiles.py)
from qublas_amd import capi
from qublas_amd.desc import CLASS_TREE, Qcomplex, Qu, RealComplexMul, RND, SAT, TRN, WRP, Tags, lower

pytestmark = pytest.mark.gpu

E43 = Qu(4, 3)
C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))   # configuration 5's element
CW = Qcomplex(Qu(14, 3), Qu(14, 3))
# name: (C element, lowering keywords).  "default": both products and every level in (6, 3); "wide": rounding products, level types
# that hold every sum; "kinds": value-dependent roundings, wrapping / zeroing overflows, converting level buffers
VARIANTS = {
    "default": (CW, dict()),
    "wide": (Qcomplex(Qu(18, 3), Qu(18, 0)), dict(mul_args=RealComplexMul(realT=Qu(8, 3, True, RND.POS_INF), imagT=Qu(8, 0)),
                                                 add_args=[Qcomplex(Qu(18, 3), Qu(18, 0))])),
    "kinds": (CW, dict(mul_args=(Qu(7, 5, True, RND.ZERO, SAT.SMGN), Qu(9, -1, True, TRN.SMGN, WRP.TCPL)),
                       add_args=[Qcomplex(Qu(8, 4, True, RND.CONV, SAT.SMGN), Qu(9, 1, True, TRN.SMGN, SAT.ZERO)),
                                 Qcomplex(Qu(12, 2, True, RND.ZERO), Qu(12, 3, True, RND.INF, WRP.TCPL))])),
}
SHAPES = [(33, 17, k, False) for k in (1, 5, 31, 32, 33, 1000)] + [(65, 40, k, False) for k in (1, 5, 31, 32, 33, 1000)] + \
         [(8, 8, 4096, False), (4, 4, 8192, False), (33, 17, 33, True), (33, 17, 5, True), (65, 40, 1000, True)]
EDGE_SHAPES = [(33, 17, 33, False), (65, 40, 1000, False)]   # at the edge-heavy operand distribution (dist 2)


def mixed_desc(variant, order, M, N, K, ta=False):
    ec, kw = VARIANTS[variant]
    ea, eb = (E43, C5) if order == "ra" else (C5, E43)
    return lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)


@functools.lru_cache(maxsize=None)
def checked(variant, order, M, N, K, ta, dist=0):
    """(descriptor, A, B, checker's C), computed once for every flag set (not modified by the callers)"""
    from oracle import qoracle
    d = mixed_desc(variant, order, M, N, K, ta)
    ea, eb, _ = R.elems(d)
    A, B = qoracle.fill(ea, M * K, 11 + K, dist), qoracle.fill(eb, K * N, 12 + K, dist)
    return d, A, B, R.gemm(d, A, B)


def run(oracle, d, A, B, **kw):
    _, _, ec = R.elems(d)
    return capi.run(d, np.zeros((kw.get("ldc") or d.M) * d.N, dtype=oracle.host_dtype(ec)), A, B, **kw)


@pytest.mark.parametrize("j", R.cases(), ids=lambda j: j["name"])
def test_golden_records_one_shot(oracle, j):
    d, A, B, exp = R.case_checked(j["name"])
    assert exp.tobytes() == R.case_expected(j).tobytes()
    assert R.strong(d, exp) or "saturation" in j["name"]
    assert run(oracle, d, A, B).tobytes() == exp.tobytes(), j["name"]


@pytest.mark.parametrize("j", R.cases(), ids=lambda j: j["name"])
def test_golden_records_second_opinions(oracle, j):
    """each reference-made record (its default plan runs in test_golden_records_one_shot) on the run-time-mode steps and on the general
    kernel's part-wise branch, and the linear-class ones on the tree kernels: all must give the reference's C"""
    d, A, B, _ = R.case_checked(j["name"])
    exp = R.case_expected(j)
    flags = [capi.OPT_RUNTIME_MODES, capi.OPT_GENERIC_TREE]
    if capi.KERNEL_NAMES[capi.classify(d).kernel] == "mfma_rc":
        flags.append(capi.OPT_FORCE_TREE)
    for fl in flags:
        assert run(oracle, d, A, B, flags=fl).tobytes() == exp.tobytes(), (j["name"], fl)


def resident(oracle, ctx, d, A, B, flags=0, lda=0, ldb=0, ldc=0):
    """pack, execute, unpack through the resident entry points; returns (plan, packed C, host C) — the caller closes the plan"""
    _, _, ec = R.elems(d)
    plan = capi.Plan(ctx, d, flags)
    pb = plan.info.packed_bytes
    pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
    dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
    ctx.h2d(dA, A)
    ctx.h2d(dB, B)
    plan.pack(capi.OPERAND_A, dA, pA, lda)
    plan.pack(capi.OPERAND_B, dB, pB, ldb)
    plan.execute(pC, pA, pB)
    host = np.zeros((ldc or d.M) * d.N, dtype=oracle.host_dtype(ec))
    host.view(np.uint8)[:] = 0xA5   # poison: bytes between the columns must survive
    dC = ctx.alloc(host.nbytes)
    ctx.h2d(dC, host)
    plan.unpack_c(pC, dC, ldc)
    ctx.d2h(host, dC)
    for p in (pA, pB, dA, dB, dC):
        ctx.free(p)
    return plan, pC, host


@pytest.mark.parametrize("j", R.cases(), ids=lambda j: j["name"])
def test_golden_records_resident(oracle, j):
    d, A, B, exp = R.case_checked(j["name"])
    with capi.Context() as ctx:
        plan, pC, got = resident(oracle, ctx, d, A, B)
        info = plan.info
        plan.close()
        ctx.free(pC)
    assert got.tobytes() == exp.tobytes(), j["name"]
    real_a = d.cmul == 3
    assert (info.host_elem_bytes[0] == 4) == real_a and (info.host_elem_bytes[1] == 4) == (not real_a)


@pytest.mark.parametrize("flags", [0, capi.OPT_RUNTIME_MODES, capi.OPT_GENERIC_TREE], ids=["default", "runtime_modes", "generic_tree"])
@pytest.mark.parametrize("order", ["ra", "rb"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tree_kernels(oracle, variant, order, flags):
    for M, N, K, ta, dist in [s + (0,) for s in SHAPES] + [s + (2,) for s in EDGE_SHAPES]:
        d, A, B, exp = checked(variant, order, M, N, K, ta, dist)
        assert R.strong(d, exp), (variant, M, N, K, dist)
        info = capi.classify(d, flags)
        # the mixed kernel: compact steps where every step is "add a constant, shift, clamp", run-time modes otherwise (built for at
        # most 12 levels); QG_OPT_GENERIC_TREE and longer run-time-mode trees: the general kernel's part-wise product branch
        runtime = variant == "kinds" or flags == capi.OPT_RUNTIME_MODES
        want = "tree_cplx" if flags == capi.OPT_GENERIC_TREE or (runtime and K > 4096) else "tree_rc_i32"
        assert info.cls == CLASS_TREE and capi.KERNEL_NAMES[info.kernel] == want, (variant, K, capi.KERNEL_NAMES[info.kernel])
        if want == "tree_rc_i32":
            assert info.reason.decode().endswith("run-time modes" if runtime else "fixed modes, compact"), info.reason
        got = run(oracle, d, A, B, flags=flags)
        assert got.tobytes() == exp.tobytes(), (variant, order, flags, M, N, K, ta, dist)


@pytest.mark.parametrize("order", ["ra", "rb"])
@pytest.mark.parametrize("variant", list(LINEAR))
def test_linear_class(oracle, variant, order):
    er, ez, ec, kw = LINEAR[variant]
    ea, eb = (er, ez) if order == "ra" else (ez, er)
    limbs = int(variant[-1])
    for M, N, K, ta in ((33, 17, 40, False), (130, 70, 200, False), (33, 17, 40, True)):
        d = lower(ea, eb, ec, M, N, K, transposed_a=ta, **kw)
        info = capi.classify(d)
        assert capi.KERNEL_NAMES[info.kernel] == "mfma_rc" and list(info.limbs) == [limbs, limbs], (info.reason, list(info.limbs))
        A, B = oracle.fill(ea, M * K, 41), oracle.fill(eb, K * N, 42)
        exp = R.gemm(d, A, B)
        assert R.strong(d, exp)
        assert run(oracle, d, A, B).tobytes() == exp.tobytes(), (variant, order, M, N, K, ta)
        # the same descriptor on the tree kernels
        assert capi.KERNEL_NAMES[capi.classify(d, capi.OPT_FORCE_TREE).kernel] in ("tree_rc_i32", "tree_cplx")
        assert run(oracle, d, A, B, flags=capi.OPT_FORCE_TREE).tobytes() == exp.tobytes(), (variant, order, M, N, K, ta, "tree")


@pytest.mark.parametrize("order", ["ra", "rb"])
def test_linear_class_saturating_narrow_c(oracle, order):
    """the labelled saturation case of the linear class: exact sums into a C far too narrow for them"""
    er, ez, _, kw = LINEAR["limb2"]
    ea, eb = (er, ez) if order == "ra" else (ez, er)
    d = lower(ea, eb, Qcomplex(Qu(6, 3), Qu(6, 0)), 130, 70, 200, **kw)
    assert capi.KERNEL_NAMES[capi.classify(d).kernel] == "mfma_rc"
    A, B = oracle.fill(ea, 130 * 200, 43), oracle.fill(eb, 200 * 70, 44)
    exp = R.gemm(d, A, B)
    assert not R.strong(d, exp)
    assert run(oracle, d, A, B).tobytes() == exp.tobytes()


@pytest.mark.parametrize("order", ["ra", "rb"])
@pytest.mark.parametrize("variant", ["tree", "linear"])
def test_check_range_host_c_and_time_execute(oracle, variant, order):
    M, N, K = 33, 17, 40
    if variant == "tree":
        d = mixed_desc("wide", order, M, N, K)
    else:
        er, ez, ec, kw = LINEAR["limb2"]
        d = lower(*((er, ez) if order == "ra" else (ez, er)), ec, M, N, K, **kw)
    ea, eb, ec = R.elems(d)
    A, B = oracle.fill(ea, M * K, 51), oracle.fill(eb, K * N, 52)
    exp = R.gemm(d, A, B)
    # QG_OPT_CHECK_RANGE: in-range operands pass, one raw value outside the real operand's format / the complex operand's imaginary
    # part is QG_ERANGE
    assert run(oracle, d, A, B, flags=capi.OPT_CHECK_RANGE).tobytes() == exp.tobytes()
    for which in ("real", "imag"):
        A2, B2 = A.copy(), B.copy()
        real_op, cplx_op = (A2, B2) if order == "ra" else (B2, A2)
        if which == "real":
            real_op[5] = (ea if order == "ra" else eb).raw_max + 1
        else:
            cplx_op["im"][7] = (eb if order == "ra" else ea).imag.raw_min - 1
        with pytest.raises(capi.QgemulError) as e:
            run(oracle, d, A2, B2, flags=capi.OPT_CHECK_RANGE)
        assert e.value.status == capi.QG_ERANGE
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d)
        pb = plan.info.packed_bytes
        pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
        dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
        ctx.h2d(dA, A)
        ctx.h2d(dB, B)
        plan.pack(capi.OPERAND_A, dA, pA)
        plan.pack(capi.OPERAND_B, dB, pB)
        assert not plan.stores_host_c                       # a complex C: through the plan's packed C and the unpack pass
        ldc = M + 3
        host = np.zeros(ldc * N, dtype=oracle.host_dtype(ec))
        host.view(np.uint8)[:] = 0xA5
        dC = ctx.alloc(host.nbytes)
        ctx.h2d(dC, host)
        plan.execute_host_c(dC, pA, pB, ldc)
        ctx.d2h(host, dC)
        grid = host.reshape(N, ldc)
        assert np.ascontiguousarray(grid[:, :M]).tobytes() == exp.tobytes()
        assert (np.ascontiguousarray(grid[:, M:]).view(np.uint8) == 0xA5).all()
        assert plan.time_execute(pC, pA, pB, 1, 3) > 0.0    # qgemul_time_execute: launches, and leaves the result of one
        got = np.zeros(M * N, dtype=oracle.host_dtype(ec))
        dG = ctx.alloc(got.nbytes)
        plan.unpack_c(pC, dG)
        ctx.d2h(got, dG)
        assert got.tobytes() == exp.tobytes()
        plan.close()
        for p in (pA, pB, pC, dA, dB, dC, dG):
            ctx.free(p)


@pytest.mark.parametrize("order", ["ra", "rb"])
def test_saturating_narrow_c_full_range(oracle, order):
    """the labelled saturation case: C is configuration 5's own narrow element, operands span their whole range"""
    ea, eb = (E43, C5) if order == "ra" else (C5, E43)
    d = lower(ea, eb, C5, 65, 40, 100)
    A, B = oracle.fill(ea, 65 * 100, 5), oracle.fill(eb, 100 * 40, 6)
    exp = R.gemm(d, A, B)
    assert not R.strong(d, exp)   # (most outputs sit at a bound of C: that is the point)
    assert run(oracle, d, A, B).tobytes() == exp.tobytes()


@pytest.mark.parametrize("order", ["ra", "rb"])
def test_128_bit_values(oracle, order):
    ea, eb = (E43, C5) if order == "ra" else (C5, E43)
    ec = Qcomplex(Qu(20, 4), Qu(20, 3))
    d = lower(ea, eb, ec, 9, 7, 37, add_args=[Qcomplex(Qu(40, 30), Qu(12, 3))])
    assert capi.KERNEL_NAMES[capi.classify(d).kernel] == "tree_i128"
    A, B = oracle.fill(ea, 9 * 37, 7), oracle.fill(eb, 37 * 7, 8)
    exp = R.gemm(d, A, B)
    assert R.strong(d, exp)
    assert run(oracle, d, A, B).tobytes() == exp.tobytes()


@pytest.mark.parametrize("order", ["ra", "rb"])
@pytest.mark.parametrize("ta", [False, True], ids=["n", "t"])
def test_leading_dimensions_with_poison(oracle, order, ta):
    M, N, K = 33, 17, 37
    d = mixed_desc("wide", order, M, N, K, ta)
    ea, eb, ec = R.elems(d)
    lda, ldb, ldc = (K if ta else M) + 3, K + 5, M + 2
    A, B = oracle.fill(ea, lda * (M if ta else K), 21), oracle.fill(eb, ldb * N, 22)   # (the gaps hold in-range values the GEMM must not read)
    tight = lambda X, ld, rows, cols: np.ascontiguousarray(X.reshape(cols, ld)[:, :rows]).reshape(-1)
    exp = R.gemm(d, tight(A, lda, K if ta else M, M if ta else K), tight(B, ldb, K, N))
    assert R.strong(d, exp)
    out = np.zeros(ldc * N, dtype=oracle.host_dtype(ec))
    out.view(np.uint8)[:] = 0xA5
    capi.run(d, out, A, B, lda=lda, ldb=ldb, ldc=ldc)
    grid = out.reshape(N, ldc)
    assert np.ascontiguousarray(grid[:, :M]).tobytes() == exp.tobytes()
    assert (np.ascontiguousarray(grid[:, M:]).view(np.uint8) == 0xA5).all()
    with capi.Context() as ctx:
        plan, pC, got = resident(oracle, ctx, d, A, B, lda=lda, ldb=ldb, ldc=ldc)
        plan.close()
        ctx.free(pC)
    assert got.tobytes() == out.tobytes()


@pytest.mark.parametrize("order", ["ra", "rb"])
def test_pack_f64_fill_and_bitstream(oracle, order):
    M, N, K = 33, 17, 37
    d = mixed_desc("wide", order, M, N, K)
    ea, eb, ec = R.elems(d)
    rng = np.random.default_rng(3)

    def doubles(e, n):   # {re, im} pairs for the complex operand, plain doubles for the real one
        return rng.uniform(-9.0, 9.0, size=n * (2 if isinstance(e, Qcomplex) else 1))

    def quantised(e, x):
        h = np.zeros(len(x) // (2 if isinstance(e, Qcomplex) else 1), dtype=oracle.host_dtype(e))
        q = lambda v, f: np.array([oracle.lib().qoracle_from_double(float(t), f.c()) for t in v], dtype=np.int64)
        if isinstance(e, Qcomplex):
            h["re"], h["im"] = q(x[0::2], e.real), q(x[1::2], e.imag)
        else:
            h[:] = q(x, e)
        return h
    xa, xb = doubles(ea, M * K), doubles(eb, K * N)
    exp = R.gemm(d, quantised(ea, xa), quantised(eb, xb))
    assert R.strong(d, exp)
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d)
        pb = plan.info.packed_bytes
        pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
        dA, dB = ctx.alloc(xa.nbytes), ctx.alloc(xb.nbytes)
        ctx.h2d(dA, xa)
        ctx.h2d(dB, xb)
        plan.pack_f64(capi.OPERAND_A, dA, pA)
        plan.pack_f64(capi.OPERAND_B, dB, pB)
        plan.execute(pC, pA, pB)
        got = np.zeros(M * N, dtype=oracle.host_dtype(ec))
        dC = ctx.alloc(got.nbytes)
        plan.unpack_c(pC, dC)
        ctx.d2h(got, dC)
        assert got.tobytes() == exp.tobytes()
        # the BitStream of that result against the oracle's
        for fmt in (capi.BITS_ASCII, capi.BITS_PACKED):
            nb = plan.bitstream_bytes(fmt)
            dBits = ctx.alloc(nb)
            plan.export_bitstream(pC, dBits, 0, 0, fmt)
            raw = np.zeros(nb, dtype=np.uint8)
            ctx.d2h(raw, dBits)
            ctx.free(dBits)
            ref = oracle.bitstream_cplx(ec, exp["re"].astype(np.int64), exp["im"].astype(np.int64), 0, 0)
            if fmt == capi.BITS_ASCII:
                assert raw.tobytes() == ref
            else:   # the packed form holds the binary digits only, not the "(", ",", " " and ")" of a complex element
                want = bytes(ch for ch in ref if ch in b"01")
                assert bytes(np.unpackbits(raw)[:len(want)] + ord("0")) == want
        # synthetic operands straight into packed form: the oracle's generator, per operand
        for dist in (0, 1):
            plan.fill(capi.OPERAND_A, 31, dist, pA)
            plan.fill(capi.OPERAND_B, 32, dist, pB)
            plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC)
            ctx.d2h(got, dC)
            assert got.tobytes() == R.gemm(d, oracle.fill(ea, M * K, 31, dist), oracle.fill(eb, K * N, 32, dist)).tobytes(), dist
        plan.close()
        for p in (pA, pB, pC, dA, dB, dC):
            ctx.free(p)


def test_run_from_two_threads(oracle):
    """each thread has its own plan cache: alternating descriptors of both orders, several calls each"""
    jobs = [checked("wide", "ra", 33, 17, 33, False), checked("kinds", "rb", 65, 40, 31, False)]
    errors = []

    def work(i):
        try:
            for rep in range(4):
                d, A, B, exp = jobs[(i + rep) % 2]
                if run(oracle, d, A, B).tobytes() != exp.tobytes():
                    errors.append((i, rep))
        except Exception as e:   # noqa: BLE001
            errors.append((i, repr(e)))
        finally:
            capi.run_release()
    ts = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(not os.path.exists(CLANG), reason="needs AMD clang (C++23)")
def test_standalone_header_runs_mixed_calls(oracle, tmp_path):
    exe = tmp_path / "amd_header_mixed_run"
    lib = os.path.join(ROOT, "qublas_amd")
    subprocess.check_call([CLANG, "-std=c++23", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "binding", "amd_header_mixed_run.cpp"),
                           "-o", str(exe), "-L" + lib, "-lqugemm", "-Wl,-rpath," + lib])
    recs = {r["name"]: r for r in (json.loads(l) for l in subprocess.check_output([str(exe)], text=True).splitlines() if l.strip())}
    assert "error" not in str(recs)
    M, N, K = 9, 7, 37

    def real(n):
        return np.array([(e * 37 + 11) % 256 - 128 for e in range(n)], dtype=np.int32)

    def cplx(n):
        h = np.zeros(n, dtype=oracle.host_dtype(C5))
        h["re"] = [(e * 53 + 7) % 1024 - 512 for e in range(n)]
        h["im"] = [(e * 5 + 3) % 16 - 8 for e in range(n)]
        return h
    calls = {"real_x_complex_default": (lower(E43, C5, CW, M, N, K), real(M * K), cplx(K * N)),
             "complex_x_real_tagged_tn": (lower(C5, E43, Qcomplex(Qu(18, 6), Qu(16, 0)), M, N, K, transposed_a=True,
                                                mul_args=RealComplexMul(realT=Qu(12, 6), imagT=Tags(10, 0))), cplx(K * M), real(K * N))}
    for name, (d, A, B) in calls.items():
        exp = R.gemm(d, A, B)
        assert R.strong(d, exp)
        got = np.asarray(recs[name]["C"], dtype=np.int64)
        assert np.array_equal(got[0::2], exp["re"].astype(np.int64)) and np.array_equal(got[1::2], exp["im"].astype(np.int64)), name
