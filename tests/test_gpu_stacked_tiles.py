"""GPU parity of the stacked linear plans — mfma_rc (real x complex: one real limb GEMM on A x [B_re | B_im] or [A_re; A_im] x B and
k_rc_convert) and mfma_cplx (complex x complex: [A_re; A_im] x [B_re | B_im] and k_cplx_combine) — on EVERY MFMA tile form their
geometry can take (tests/stacked_cases.py; tests/test_stacked_tile_coverage.py pins each case to its kernel variant on the CPU):
64 x 64, 128 x 128 on 64- and 128-byte k-tiles, the 256 x 256 two-group kernel, the row-step limb kernel and the persistent limb
kernels, on launches of many tiles, at uniform (dist 0) and edge-heavy (dist 2) operands, byte for byte.
  * against the oracle (tests/mixed_ref.py, oracle/qoracle.c) on bands of C placed by the plan's tile: the first 8 rows, the 8 around
    the first interior tile seam, everything from 4 before the last tile's start (which holds the tiles a persistent kernel takes in its
    second round), the same for columns, each over the whole other extent; both parts of C, so both sides of the stack seam;
  * the whole matrix against the same descriptor on the tree kernels (QG_OPT_FORCE_TREE), which their own tests pin to the oracle:
    a wrong tile in the interior;
  * the device's plane-mask dispatch of a stacked 3 x 3 plan; the resident entry points with leading dimensions.
Strength: at least half of each part's compared outputs are neither zero nor at a bound of C; at dist 2 the minimum and the maximum of
every operand part occur in the rows / columns that feed the compared bands."""
import functools

import numpy as np
import pytest

import mixed_ref as R
import stacked_cases as S
from qublas_amd import capi
from qublas_amd.desc import Qcomplex
from test_gpu_mixed import resident, run

pytestmark = pytest.mark.gpu

TREE_KERNELS = ("tree_rc_i32", "tree_cplx_i32", "tree_cplx", "tree_i128")


def reference_gemm(d, A, B, ec, rows, cols, out):
    from oracle import qoracle
    if R.is_mixed(d):
        R.gemm(d, A, B, rows=rows, cols=cols, nthreads=16, out=out)
    else:
        qoracle.gemm(d, A, B, ec, rows=rows, cols=cols, nthreads=16, out=out)


def banded(d, A, B, tile):
    """(oracle's C, zero outside the bands; mask [N][M] of the bands) for tiles of `tile` x `tile`"""
    from oracle import qoracle
    _, _, ec = R.elems(d)
    assert S.oracle_cost(S.KERNEL_RC if R.is_mixed(d) else S.KERNEL_CPLX, d.M, d.N, d.K, tile, tile) <= S.COST_CAP
    exp = np.zeros(d.M * d.N, dtype=qoracle.host_dtype(ec))
    mask = np.zeros((d.N, d.M), dtype=bool)
    for r, c in S.blocks(d.M, d.N, tile, tile):
        reference_gemm(d, A, B, ec, r, c, exp)
        mask[c[0]:c[1], r[0]:r[1]] = True
    return exp, mask


@functools.lru_cache(maxsize=2)
def reference(name, dist):
    """(descriptor, A, B, oracle's bands, mask) of a table case, computed once (not modified by the callers)"""
    from oracle import qoracle
    c = S.BY_NAME[name]
    d = S.desc(c)
    ea, eb, _ = R.elems(d)
    A, B = qoracle.fill(ea, d.M * d.K, 61, dist), qoracle.fill(eb, d.K * d.N, 62, dist)
    return (d, A, B) + banded(d, A, B, S.VARIANTS[c.variant][2])


def differing(a, b):
    """{part: (how many elements differ, the first such index)} of two host-layout complex arrays; empty where they are equal"""
    assert a.shape == b.shape and a.dtype == b.dtype
    bad = {n: np.flatnonzero(a[n] != b[n]) for n in a.dtype.names}
    return {n: (len(i), int(i[0])) for n, i in bad.items() if len(i)}


def differing_in_bands(got, exp, mask, M, N):
    return differing(got.reshape(N, M)[mask], exp.reshape(N, M)[mask])


def parts(e):
    return (("re", e.real), ("im", e.imag)) if isinstance(e, Qcomplex) else ((None, e),)


def edge_witness(d, A, B, mask):
    """the minimum and the maximum of every operand part occur in a row of A / a column of B that feeds a compared row / column band"""
    ea, eb, _ = R.elems(d)
    # (a row band is a row of the mask that is set over every column, and the other way round)
    rows, cols = mask.all(axis=0), mask.all(axis=1)
    assert rows.any() and cols.any() and not rows.all() and not cols.all()
    a = (A.reshape(d.M, d.K) if d.transA else A.reshape(d.K, d.M).T)[rows]   # [i][k]
    b = B.reshape(d.N, d.K)[cols]                                           # [j][k]
    for x, e in ((a, ea), (b, eb)):
        for name, f in parts(e):
            v = x[name] if name else x
            assert (v == f.raw_min).any() and (v == f.raw_max).any(), (str(f), name)


def check_case(oracle, d, A, B, exp, mask, dist, want_kernel, want_limbs):
    info = capi.classify(d)
    assert info.kernel == want_kernel and list(info.limbs) == list(want_limbs), (info.reason, list(info.limbs))
    assert R.strong(d, exp.reshape(d.N, d.M)[mask])
    if dist == 2:
        edge_witness(d, A, B, mask)
    got = run(oracle, d, A, B)
    assert not differing_in_bands(got, exp, mask, d.M, d.N)
    assert capi.KERNEL_NAMES[capi.classify(d, capi.OPT_FORCE_TREE).kernel] in TREE_KERNELS
    assert not differing(got, run(oracle, d, A, B, flags=capi.OPT_FORCE_TREE))
    return got


@pytest.mark.parametrize("dist", [0, 2])
@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_stacked_plan_on_its_tile_form(oracle, name, dist):
    c = S.BY_NAME[name]
    d, A, B, exp, mask = reference(name, dist)
    check_case(oracle, d, A, B, exp, mask, dist, c.kernel, c.limbs)


@pytest.mark.parametrize("which", ["two_limb_values", "imag_32640", "real_minus_32641"])
@pytest.mark.parametrize("order", ["ra", "rb"])
@pytest.mark.parametrize("shape", S.MASK_SHAPES, ids=lambda s: "%dx%dx%d" % s[:3])
def test_plane_mask_dispatch_on_a_stacked_plan(oracle, shape, order, which):
    """3 x 3-limb operands carry a plane mask, a stacked operand ONE for both parts; when the third int8 limb plane of both operands is
    empty the 2 x 2 body does the work, otherwise the 3 x 3 one — chosen on the device.  The boundary values of
    tests/test_gpu_parity.py::test_limb_plane_mask_dispatch: every value inside [-32640, 32639] (32639 is the largest two-limb value);
    one 32640 in the imaginary part only, in the last row of the stacked operand's last tile; one -32641 in the real operand only."""
    M, N, K, variant = shape
    d = S.mask_desc(order, M, N, K)
    M, N = d.M, d.N
    er, ez, _, _ = S.MASK3
    rng = np.random.default_rng(M + 7 * len(which))

    def values(n):
        x = rng.integers(-32640, 32640, n, dtype=np.int64)
        x[:2] = [32639, -32640]   # the extremes of two limbs are present
        return x
    nr, nz = (M * K, K * N) if order == "ra" else (K * N, M * K)
    real = values(nr).astype(oracle.host_dtype(er))
    cplx = np.zeros(nz, dtype=oracle.host_dtype(ez))
    cplx["re"], cplx["im"] = values(nz), values(nz)
    plain = (real.copy(), cplx.copy())
    if which == "imag_32640":
        # the complex operand's last row: B's column N - 1 (element k + (N - 1) K), A's row M - 1 (element M - 1 + k M)
        cplx["im"][nz - 1] = 32640
        assert cplx["re"].max() <= 32639 and real.max() <= 32639
    if which == "real_minus_32641":
        real[nr // 2] = -32641
        assert cplx["re"].min() >= -32640 and cplx["im"].min() >= -32640
    for real_v, cplx_v in ((real, cplx),) + (() if which == "two_limb_values" else (plain,)):
        # (then the two-limb operands again: re-packing into the SAME cached device buffers must not leave a stale mask behind)
        A, B = (real_v, cplx_v) if order == "ra" else (cplx_v, real_v)
        exp, mask = banded(d, A, B, S.VARIANTS[variant][2])
        check_case(oracle, d, A, B, exp, mask, 0, S.KERNEL_RC, (3, 3))


@pytest.mark.parametrize("name", S.RESIDENT)
def test_resident_path_with_leading_dimensions(oracle, name):
    """pack with leading dimensions, execute, unpack_c with ldc > M into a poisoned buffer: the bands against the oracle, the whole
    matrix against the one-shot call on the tree kernels, and the poison between the columns survives"""
    d, A, B, exp, mask = reference(name, 0)
    M, N, K = d.M, d.N, d.K
    ea, eb, _ = R.elems(d)
    ra, ca = (K, M) if d.transA else (M, K)   # A as stored: ca columns of ra elements
    lda, ldb, ldc = ra + 3, K + 5, M + 2
    Ap, Bp = oracle.fill(ea, lda * ca, 63), oracle.fill(eb, ldb * N, 64)   # (the gaps hold in-range values the GEMM must not read)
    Ap.reshape(ca, lda)[:, :ra] = A.reshape(ca, ra)
    Bp.reshape(N, ldb)[:, :K] = B.reshape(N, K)
    with capi.Context() as ctx:
        plan, pC, got = resident(oracle, ctx, d, Ap, Bp, lda=lda, ldb=ldb, ldc=ldc)
        kernel = plan.info.kernel
        plan.close()
        ctx.free(pC)
    assert kernel == S.BY_NAME[name].kernel
    grid = got.reshape(N, ldc)
    tight = np.ascontiguousarray(grid[:, :M]).reshape(-1)
    assert not differing_in_bands(tight, exp, mask, M, N)
    assert not differing(tight, run(oracle, d, A, B, flags=capi.OPT_FORCE_TREE))
    assert (np.ascontiguousarray(grid[:, M:]).view(np.uint8) == 0xA5).all()
