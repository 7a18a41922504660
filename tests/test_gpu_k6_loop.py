"""k_mfma_k6's k-loop (qg_mfma_k6.hip) carries its two LDS read addresses from one k-tile to the next (moved on at the end of the
MFMA interval), issues its LDS-DMA from a scalar base plus a 32-bit lane offset, and loads every row sum of a tile ahead of the
epilogue's first store.  The shapes are the smallest at which that state can go wrong: one tile of one k-tile (every refill of
the loop is a clamped one), four tiles with the ring of three buffers wrapping once, and 352 tiles on 256 persistent workgroups,
where the carried addresses and the DMA ring cross a tile boundary, with an even and an odd number of k-tiles.  The planner gives
the six-product kernel only problems with at least one 128 x 128 tile per compute unit (qg_mfma_pick: 256 of them), so the one-
and four-tile shapes run on the lock-step limb kernel, whatever the flags; they are kept as the small valid launches they are,
and each has a counterpart of the same k-tile count at the smallest size the kernel does get (2112 x 2048 and 2113 x 2049, one
row and one column into a further tile).  Every case is compared byte for byte with QG_OPT_SCHOOLBOOK_LIMBS (the nine-product
kernel) and, on the row and column windows of test_gpu_k6.py cut to the matrix, with the oracle.  Every case is a valid launch.
Run time on an MI355X: a few seconds."""
import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qu, RND, SAT, TRN, Tags, lower

pytestmark = pytest.mark.gpu

E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)     # bench.py's operand: 17 bits
KW88 = dict(mul_args=Tags(17, 16), add_args=[Qu(29, 16)])
C4 = Qu(23, 8)                               # 4-byte container, the shift-and-clamp epilogue (the headline's)
C8 = Qu(29, 16)                              # 8-byte container, the shift-and-clamp epilogue
CG = Qu(12, 8, True, RND.POS_INF, SAT.TCPL)  # not FAST: the general round + overflow routine
K6 = b"six products"


def takes_k6(M, N):
    return ((M + 127) // 128) * ((N + 127) // 128) >= 256


def run_arm(d, flags, dist, host, host_c=False):
    """device fill (or, host = (A, B): pack these host-layout operands), execute, unpack; returns the host-layout bytes of C"""
    with capi.Context() as ctx:
        plan = capi.Plan(ctx, d, flags)
        info = plan.info
        assert capi.KERNEL_NAMES[info.kernel] == "mfma_i8_limb"
        assert (K6 in bytes(info.reason)) == (flags == 0 and takes_k6(d.M, d.N)), bytes(info.reason)
        pb = info.packed_bytes
        pA, pB, pC = ctx.alloc(pb[0]), ctx.alloc(pb[1]), ctx.alloc(pb[2])
        nbytes = d.M * d.N * info.host_elem_bytes[2]
        dC = ctx.alloc(nbytes)
        if host is None:
            plan.fill(capi.OPERAND_A, 1, dist, pA)
            plan.fill(capi.OPERAND_B, 2, dist, pB)
        else:
            for op, arr, dst in ((capi.OPERAND_A, host[0], pA), (capi.OPERAND_B, host[1], pB)):
                dev = ctx.alloc(arr.nbytes)
                ctx.h2d(dev, arr)
                plan.pack(op, dev, dst)
                ctx.sync()
                ctx.free(dev)
        if host_c and takes_k6(d.M, d.N):
            assert plan.stores_host_c
        if host_c and plan.stores_host_c:      # (the lock-step limb kernel of the small shapes has no such store: packed C + unpack)
            plan.execute_host_c(dC, pA, pB)
        else:
            plan.execute(pC, pA, pB)
            plan.unpack_c(pC, dC)
        out = np.zeros(nbytes, np.uint8)
        ctx.d2h(out, dC)
        for p in (pA, pB, pC, dC):
            ctx.free(p)
        plan.close()
    return out


def windows(M, N):
    """the windows of test_gpu_k6.test_shapes_around_the_tile, cut to an M x N matrix"""
    r = max(M - 100, 0)
    return [((0, min(8, M)), (0, min(256, N))),
            ((r, min(r + 10, M)), (max(N - 200, 0), N)),      # group 1's rows of the last-but-one tile
            ((max(M - 6, 0), M), (max(N - 130, 0), N))]       # the ragged corner


def run_case(oracle, M, N, K, ec, dist, host_c=False):
    d = lower(E88, E88, ec, M, N, K, **KW88)
    A = oracle.fill(E88, M * K, 1, dist)
    B = oracle.fill(E88, K * N, 2, dist)
    host = (A, B) if dist == 2 else None      # the edge set exists on the host only
    got = run_arm(d, 0, dist, host, host_c)
    nine = run_arm(d, capi.OPT_SCHOOLBOOK_LIMBS, dist, host)
    assert np.array_equal(got, nine), "six products differ from QG_OPT_SCHOOLBOOK_LIMBS"
    cdt = oracle.host_dtype(ec)
    for rows, cols in windows(M, N):
        exp = np.zeros(M * N, dtype=cdt)
        oracle.gemm(d, A, B, ec, rows=rows, cols=cols, nthreads=16, out=exp)
        sl = (slice(cols[0], cols[1]), slice(rows[0], rows[1]))
        assert np.array_equal(got.view(cdt).reshape(N, M)[sl], exp.reshape(N, M)[sl]), (rows, cols)


@pytest.mark.parametrize("M,N,K", [
    (96, 128, 64),         # one tile, one k-tile
    (97, 129, 192),        # four tiles, three k-tiles
    (2112, 2048, 64),      # the six-product kernel, one k-tile: every refill of the loop is a clamped one
    (2113, 2049, 192),     # three k-tiles: the ring wraps once per tile; ragged last tiles
    (2112, 2048, 128),     # 352 tiles on 256 workgroups: the carried LDS addresses and the DMA ring cross a tile boundary
    (2112, 2048, 320),     # odd number of k-tiles
])
def test_shapes(oracle, M, N, K):
    run_case(oracle, M, N, K, C4, 0)


@pytest.mark.parametrize("ec,dist,host_c", [
    (C4, 2, False),        # the edge operands
    (C8, 0, False),        # 8-byte container
    (C8, 2, False),
    (CG, 0, False),        # the general routine behind the recombination
    (C4, 0, True),         # the host-layout store
    (C8, 2, True),
], ids=["c4-edge", "c8", "c8-edge", "pos_inf", "c4-host", "c8-edge-host"])
@pytest.mark.parametrize("M,N", [(97, 129), (2113, 2049)])
def test_three_k_tiles_every_epilogue(oracle, M, N, ec, dist, host_c):
    run_case(oracle, M, N, 192, ec, dist, host_c)
