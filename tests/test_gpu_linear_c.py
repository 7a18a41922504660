"""Every conversion site of the linear class at C's ties and bounds, on designed dot products.

In the linear class the dot product is exact and the one place where rounding and overflow happen is the conversion sum -> C, written out
in every MFMA kernel's epilogue and in the conversion passes.  tests/designed_sums.py builds operands whose exact dot product is
prescribed per output element, s(i, j) = centres[(i + ri) % P] + offsets[(j + rj) % Q] with P and Q odd, coprime and dividing no tile
extent, so ties of both signs and parities, hi, hi + 1, lo, lo - 1, -hi, 0, -1 and multiple wraps stand at every row-in-run and lane
position of every tile; tests/linear_c_cases.py crosses every site with about ten C formats per container (all seven QuModes, all four
OfModes, the shift-and-clamp pair and its neighbours, d = 1, a deep shift, d = 0, a left shift, an unsigned C), and
tests/test_linear_c_coverage.py pins on the CPU that each case reaches its kernel and that the witnesses and shares hold.  Here, per case:
  * C over the WHOLE matrix equals the expectation — the oracle's scalar conversion of the P x Q designed sums, tiled;
  * the oracle's GEMM on the bands of the plan's tile (first rows, first interior seam, last tile; the same for columns) equals both;
  * the second kernel of the same descriptor gives the same bytes: the tree class on the small shapes (QG_OPT_FORCE_TREE), the plain
    balanced limbs of a centred plan (QG_OPT_BALANCED_LIMBS); the lock-step 256 x 256 form (QG_OPT_LOCKSTEP_TILES) and the nine-product
    kernel (QG_OPT_SCHOOLBOOK_LIMBS) are sites of their own on the descriptors of k_mfma_pp and of the six-product kernel;
  * the kernels that can store the reference layout (k_mfma_pp, k_mfma_ppl / ppl22, k_mfma_k6 with a 4- or 8-byte C) run all three
    stores: the one-shot call (leading dimension M, odd), the packed store + unpack, and qgemul_execute_host_c with padded leading
    dimensions whose gaps must survive — M + 3, a multiple of 4 (the vector-store branch), and M + 2, odd (the scalar-store branch);
  * batched (block-diagonal) and grouped launches: three members of different phase (grouped: of different shape), each against its own
    expectation and against its plain plan;
  * the stacked plans' second passes (k_cplx_combine, k_rc_convert; as three members of a stacked block-diagonal batch,
    k_stack_combine_bd): A's parts carry two centre lists, the parts of C two different formats; also against the tree class.
A failure reports the (centre, offset) classes and the tile-local positions that differ.

Run time on an MI355X, host work included: 993 tests in 40 s; the slowest case 0.24 s (the first one: it loads the library), the
4105 x 3853 cases of the 256 x 256 kernels 0.17 to 0.21 s each."""
import numpy as np
import pytest

import designed_sums as DS
import linear_c_cases as L
from qublas_amd import capi
from qublas_amd.desc import lower

pytestmark = pytest.mark.gpu

KERNEL = {True: "mfma_i8", False: "mfma_i8_limb"}
HOST_C_VARIANTS = (9, 10, 11)


def run(oracle, d, ec, A, B, flags=0):
    return capi.run(d, np.zeros(d.M * d.N, dtype=oracle.host_dtype(ec)), A, B, flags=flags)


def band_mask(M, N, TM, TN):
    mask = np.zeros((N, M), dtype=bool)
    for r, c in L.band_blocks(M, N, TM, TN):
        mask[c[0]:c[1], r[0]:r[1]] = True
    return mask


def oracle_bands(oracle, d, ec, A, B, TM, TN):
    exp = np.zeros(d.M * d.N, dtype=oracle.host_dtype(ec))
    for r, c in L.band_blocks(d.M, d.N, TM, TN):
        oracle.gemm(d, A, B, ec, rows=r, cols=c, nthreads=16, out=exp)
    return exp


def resident_stores(oracle, d, ec, A, B, flags):
    """(packed store + unpack, [(qgemul_execute_host_c into a poisoned buffer, ldc)]) of a plan that stores the host layout: ldc = M + 3,
    a multiple of 4 on every such site (the vector-store branch), and ldc = M + 2, odd (the scalar-store branch)"""
    dt = oracle.host_dtype(ec)
    assert d.M % 2 == 1 and (d.M + 3) % 4 == 0
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, flags)
        assert plan.stores_host_c
        pb = plan.info.packed_bytes
        pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
        dA, dB = ctx.alloc(A.nbytes), ctx.alloc(B.nbytes)
        ctx.h2d(dA, A)
        ctx.h2d(dB, B)
        plan.pack(capi.OPERAND_A, dA, pA)
        plan.pack(capi.OPERAND_B, dB, pB)
        packed = np.zeros(d.M * d.N, dtype=dt)
        dC = ctx.alloc(packed.nbytes)
        plan.execute(pC, pA, pB)
        plan.unpack_c(pC, dC)
        ctx.d2h(packed, dC)
        hosts = []
        for ldc in (d.M + 3, d.M + 2):
            host = np.zeros(ldc * d.N, dtype=dt)
            host.view(np.uint8)[:] = 0xA5
            hC = ctx.alloc(host.nbytes)
            ctx.h2d(hC, host)
            plan.execute_host_c(hC, pA, pB, ldc)
            ctx.d2h(host, hC)
            ctx.free(hC)
            hosts.append((host, ldc))
        for p in (pA, pB, pC, dA, dB, dC):
            ctx.free(p)
        plan.close()
    return packed, hosts


@pytest.mark.parametrize("name", [c.name for c in L.CASES])
def test_designed_sums_on_every_conversion_site(oracle, name):
    c = L.BY_NAME[name]
    s, (ea, eb, es), _, _, _ = L.plan(c)
    d, dz = L.designed(oracle, c)
    M, N = s.M, s.N
    TM, TN = L.VARIANTS[s.variant][2:]
    info = capi.classify(d, s.flags)
    assert capi.KERNEL_NAMES[info.kernel] == KERNEL[s.limbs == (1, 1) and s.variant != 12] and tuple(info.limbs) == s.limbs, (info.reason, list(info.limbs))
    exp = DS.expectation(oracle, dz, es, c.ec, M, N)
    got = run(oracle, d, c.ec, dz.A, dz.B, s.flags)
    assert np.array_equal(got, exp), name + "\n" + DS.report(dz, got, exp, M, N, TM)
    mask = band_mask(M, N, TM, TN).reshape(-1)
    bands = oracle_bands(oracle, d, c.ec, dz.A, dz.B, TM, TN)
    assert np.array_equal(bands[mask], exp[mask]), name + " (oracle GEMM against the designed expectation)\n" + DS.report(dz, np.where(mask, bands, exp), exp, M, N, TM)
    assert np.array_equal(bands[mask], got[mask])
    for fl in s.second:
        info2 = capi.classify(d, fl)
        assert fl != capi.OPT_FORCE_TREE or capi.KERNEL_NAMES[info2.kernel].startswith("tree"), info2.reason
        # (the plain balanced limbs of a centred plan: one limb more per operand, so another kernel body or another instantiation)
        assert fl != capi.OPT_BALANCED_LIMBS or tuple(info2.limbs) != tuple(info.limbs), (list(info2.limbs), info2.reason)
        other = run(oracle, d, c.ec, dz.A, dz.B, fl)
        assert np.array_equal(other, got), "%s flags %d\n%s" % (name, fl, DS.report(dz, other, exp, M, N, TM))
    if s.variant in HOST_C_VARIANTS and L.expected(c)["container"] in (4, 8) and not L.expected(c)["comp"] and not L.expected(c)["wide_ep"]:
        packed, hosts = resident_stores(oracle, d, c.ec, dz.A, dz.B, s.flags)
        assert np.array_equal(packed, exp), name + " (packed store)\n" + DS.report(dz, packed, exp, M, N, TM)
        for host, ldc in hosts:
            grid = host.reshape(N, ldc)
            tight = np.ascontiguousarray(grid[:, :M]).reshape(-1)
            assert np.array_equal(tight, exp), "%s (host-layout store, ldc = %d)\n%s" % (name, ldc, DS.report(dz, tight, exp, M, N, TM))
            assert (np.ascontiguousarray(grid[:, M:]).view(np.uint8) == 0xA5).all(), (name, ldc)


# ---- batched (block-diagonal) and grouped launches: the same epilogue code on BD / GRP tile bases
MEMBER_SITES = ("k64", "limb64_33")
MEMBER_CASES = [c.name for c in L.CASES if c.site in MEMBER_SITES and c.container in (1, 4)]
GROUP_SHAPES = [(137, 77), (73, 141), (201, 13)]


def member_operands(oracle, c, shapes, K):
    """[(descriptor, Designed, expectation)] of members with the case's designed sums at different phases (and shapes)"""
    s, (ea, eb, es), centres, offsets, _ = L.plan(c)
    out = []
    for m, (M, N) in enumerate(shapes):
        dz = DS.build(oracle, ea, eb, es, M, N, K, centres, offsets, ri=(5 * m + c.idx) % len(centres), rj=(3 * m + 2 * c.idx) % len(offsets), transposed_a=c.ta)
        d = lower(ea, eb, c.ec, M, N, K, mul_args=L.OPERANDS[s.op][2], add_args=[es], transposed_a=c.ta)
        out.append((d, dz, DS.expectation(oracle, dz, es, c.ec, M, N)))
    return out


@pytest.mark.parametrize("name", MEMBER_CASES)
def test_batched_members_of_different_phase(oracle, name):
    c = L.BY_NAME[name]
    s, _, _, _, K = L.plan(c)
    members = member_operands(oracle, c, [(s.M, s.N)] * 3, K)
    d = members[0][0]
    assert capi.classify_batched_launches(d, 3) == 1   # the block-diagonal form
    A = np.concatenate([m[1].A for m in members])
    B = np.concatenate([m[1].B for m in members])
    got = capi.run_batched(d, 3, np.zeros(3 * s.M * s.N, dtype=oracle.host_dtype(c.ec)), A, B, s.M * s.N, s.M * K, K * s.N)
    for m, (dm, dz, exp) in enumerate(members):
        part = got[m * s.M * s.N:(m + 1) * s.M * s.N]
        assert np.array_equal(part, exp), "%s member %d\n%s" % (name, m, DS.report(dz, part, exp, s.M, s.N, 64))
        assert np.array_equal(part, run(oracle, dm, c.ec, dz.A, dz.B))   # the plain plan of the member


@pytest.mark.parametrize("name", MEMBER_CASES)
def test_grouped_members_of_different_shape(oracle, name):
    c = L.BY_NAME[name]
    _, _, _, _, K = L.plan(c)
    members = member_operands(oracle, c, GROUP_SHAPES, K)
    descs = [m[0] for m in members]
    assert capi.classify_grouped_launches(descs) == 1 and all(capi.classify_grouped_member(descs, g).in_launch for g in range(3))
    Cs = [np.zeros(d.M * d.N, dtype=oracle.host_dtype(c.ec)) for d in descs]
    capi.run_grouped(descs, Cs, [m[1].A for m in members], [m[1].B for m in members])
    for g, (dm, dz, exp) in enumerate(members):
        assert np.array_equal(Cs[g], exp), "%s member %d\n%s" % (name, g, DS.report(dz, Cs[g], exp, dm.M, dm.N, 64))
        assert np.array_equal(Cs[g], run(oracle, dm, c.ec, dz.A, dz.B))


# ---- the second passes of the stacked plans: k_cplx_combine (complex x complex), k_rc_convert (complex x real) and, behind the stacked
# block-diagonal batch, k_stack_combine_bd.  A's parts carry two centre lists, the parts of C two different formats
def stacked_expectation(oracle, c, dr, di):
    _, _, _, es = L.stacked_operands(c.kind)
    M, N = L.STACKED_SHAPE
    exp = np.zeros(M * N, dtype=oracle.host_dtype(c.ec))
    exp["re"] = DS.expectation(oracle, dr, es.real, c.ec.real, M, N)
    exp["im"] = DS.expectation(oracle, di, es.imag, c.ec.imag, M, N)
    return exp


def stacked_report(dr, di, got, exp):
    M, N = L.STACKED_SHAPE
    return "\n".join("%s part:\n%s" % (p, DS.report(dz, np.ascontiguousarray(got[p]), np.ascontiguousarray(exp[p]), M, N, 64))
                     for p, dz in (("re", dr), ("im", di)) if not np.array_equal(got[p], exp[p]))


@pytest.mark.parametrize("name", [c.name for c in L.STACKED_CASES])
def test_stacked_second_passes(oracle, name):
    c = L.STACKED_BY_NAME[name]
    M, N = L.STACKED_SHAPE
    members = [L.stacked_designed(oracle, c, m) for m in range(3)]
    d, A, B, dr, di = members[0]
    dt = oracle.host_dtype(c.ec)
    assert capi.KERNEL_NAMES[capi.classify(d).kernel] == ("mfma_cplx" if c.kind == "cc" else "mfma_rc")
    exp = stacked_expectation(oracle, c, dr, di)
    got = capi.run(d, np.zeros(M * N, dtype=dt), A, B)
    assert np.array_equal(got, exp), name + "\n" + stacked_report(dr, di, got, exp)
    assert capi.KERNEL_NAMES[capi.classify(d, capi.OPT_FORCE_TREE).kernel].startswith("tree")
    tree = capi.run(d, np.zeros(M * N, dtype=dt), A, B, flags=capi.OPT_FORCE_TREE)
    assert np.array_equal(tree, got), name + " (tree class)\n" + stacked_report(dr, di, tree, exp)
    # three members of different phase in the stacked block-diagonal batch: one launch and one combine pass
    assert capi.classify_batched_launches(d, 3, capi.OPT_BATCHED_STACKED) == 2
    K = d.K
    out = capi.run_batched(d, 3, np.zeros(3 * M * N, dtype=dt), np.concatenate([m[1] for m in members]), np.concatenate([m[2] for m in members]),
                           M * N, M * K, K * N, flags=capi.OPT_BATCHED_STACKED)
    for m, (_, _, _, mr, mi) in enumerate(members):
        part, want = out[m * M * N:(m + 1) * M * N], stacked_expectation(oracle, c, mr, mi)
        assert np.array_equal(part, want), "%s member %d\n%s" % (name, m, stacked_report(mr, mi, part, want))
