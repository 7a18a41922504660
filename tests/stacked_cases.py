"""The case table of the stacked linear plans — TEST INFRASTRUCTURE, not a test module.

mfma_rc (real x complex) and mfma_cplx (complex x complex) run ONE real limb GEMM on operands whose parts are stacked along the rows and a
second pass over the raw 64-bit dot products; the tile geometry comes from qg_mfma_pick on the stacked extents, so either plan can land on
any MFMA kernel.  CASES names, per case, the kernel variant (QMfmaCfg::variant, qublas_amd/csrc/qg_geom.h), the limb counts and the plan's
kernel it must reach; tests/test_stacked_tile_coverage.py pins those through the planner driver on the CPU and
tests/test_gpu_stacked_tiles.py runs every case on the GPU.  The element and tag definitions of the other linear-class tests of these two
plans live here too (LINEAR: tests/test_gpu_mixed.py; C5 / BL / LW / C8 / B8 / L8: tests/test_gpu_parity.py)."""
from collections import namedtuple

from qublas_amd.desc import BasicComplexMul, Qcomplex, Qu, RealComplexMul, RND, SAT, lower

KERNEL_RC, KERNEL_CPLX = 12, 7   # QG_KERNEL_MFMA_RC, QG_KERNEL_MFMA_CPLX (include/qgemul.h)
# QMfmaCfg::variant -> (enumerator, BK, TM = TN); the variants qg_mfma_pick returns
VARIANTS = {1: ("QG_MFMA_128", 64, 128), 3: ("QG_MFMA_LIMB_128", 64, 128), 6: ("QG_MFMA_LIMB_64", 64, 64), 7: ("QG_MFMA_64_BK128", 128, 64),
            8: ("QG_MFMA_128_BK128", 128, 128), 9: ("QG_MFMA_PP", 128, 256), 10: ("QG_MFMA_PPL", 64, 128)}
PERSISTENT = {9, 10}
COST_CAP = 1.5e8   # part-MACs of oracle work per test

C5 = Qcomplex(Qu(6, 3, True, RND.POS_INF, SAT.TCPL), Qu(6, -3, True, RND.POS_INF, SAT.TCPL))   # configuration 5's element

# ---- real x complex.  name: (real element, complex element, C, lowering keywords): products with one spare bit and level types that hold
# every sum, so nothing rounds or overflows before C; C's parts have fewer fraction bits than the products (right shifts of 2 and 1, 3 and
# 3, 6 and 0)
LINEAR = {
    "limb1": (Qu(4, 3), Qcomplex(Qu(4, 3), Qu(4, 1)), Qcomplex(Qu(18, 4), Qu(18, 3)),
              dict(mul_args=RealComplexMul(realT=Qu(10, 6), imagT=Qu(10, 4)), add_args=[Qcomplex(Qu(18, 6), Qu(18, 4))])),
    "limb2": (Qu(6, 6), C5, Qcomplex(Qu(22, 6), Qu(22, 0)),
              dict(mul_args=RealComplexMul(realT=Qu(14, 9), imagT=Qu(14, 3)), add_args=[Qcomplex(Qu(22, 9), Qu(22, 3))])),
    "limb3": (Qu(8, 8), Qcomplex(Qu(8, 8), Qu(7, 5)), Qcomplex(Qu(26, 10), Qu(25, 13)),
              dict(mul_args=RealComplexMul(realT=Qu(18, 16), imagT=Qu(17, 13)), add_args=[Qcomplex(Qu(26, 16), Qu(25, 13))])),
}
# unequal limb counts (shifts of 3 and 2, 3 and 2): 8-bit real coefficients x 16-bit I/Q samples, 1 x 3 limbs; x 15-bit samples (14 value
# bits and the sign: the largest two-limb value is 32639), 1 x 2 limbs
UNEQUAL = {
    "limb13": (Qu(4, 3), Qcomplex(Qu(7, 8), Qu(7, 8)), Qcomplex(Qu(22, 8), Qu(22, 9)),
               dict(mul_args=RealComplexMul(realT=Qu(13, 11), imagT=Qu(13, 11)), add_args=[Qcomplex(Qu(22, 11), Qu(22, 11))])),
    "limb12": (Qu(4, 3), Qcomplex(Qu(7, 7), Qu(6, 8)), Qcomplex(Qu(22, 7), Qu(21, 9)),
               dict(mul_args=RealComplexMul(realT=Qu(13, 10), imagT=Qu(12, 11)), add_args=[Qcomplex(Qu(22, 10), Qu(21, 11))])),
}
# the plane-mask cases: 3 x 3 limbs where BOTH parts of the complex operand hold 32640 (LINEAR's limb3 has a 13-bit imaginary part)
MASK3 = (Qu(8, 8), Qcomplex(Qu(8, 8), Qu(8, 8)), Qcomplex(Qu(26, 10), Qu(26, 13)),
         dict(mul_args=RealComplexMul(realT=Qu(18, 16), imagT=Qu(18, 16)), add_args=[Qcomplex(Qu(26, 16), Qu(26, 16))]))

# ---- complex x complex: BasicComplexMul sub-ops and tree levels that are all exact.  name: (element, C, lowering keywords)
BL = BasicComplexMul(acT=Qu(14, 6), bdT=Qu(14, -6), adT=Qu(14, 0), bcT=Qu(14, 0), acbdT=Qu(15, 6), adbcT=Qu(15, 0))
LW = Qcomplex(Qu(30, 6), Qu(30, 0))
# symmetric 8-bit parts: single limb per part
C8 = Qcomplex(Qu(4, 3), Qu(4, 3))
# adbcT needs 11 int bits: ad + bc reaches exactly 2^15 at a=b=c=d=-128, and two of those overflow Qu<10,6> by one LSB
B8 = BasicComplexMul(acT=Qu(9, 6), bdT=Qu(9, 6), adT=Qu(9, 6), bcT=Qu(9, 6), acbdT=Qu(11, 6), adbcT=Qu(11, 6))
L8 = Qcomplex(Qu(22, 6), Qu(22, 6))
# 17-bit parts: 3 x 3 limbs
C17 = Qcomplex(Qu(8, 8), Qu(8, 8))
B17 = BasicComplexMul(acT=Qu(18, 16), bdT=Qu(18, 16), adT=Qu(18, 16), bcT=Qu(18, 16), acbdT=Qu(19, 16), adbcT=Qu(19, 16))
L17 = Qcomplex(Qu(28, 16), Qu(28, 16))
COMPLEX = {
    "limb1": (C8, Qcomplex(Qu(19, 3), Qu(19, 4)), dict(mul_args=B8, add_args=[L8])),
    "limb2": (C5, Qcomplex(Qu(20, 4, True, RND.POS_INF), Qu(20, 0)), dict(mul_args=BL, add_args=[LW])),
    "limb3": (C17, Qcomplex(Qu(28, 10), Qu(28, 12)), dict(mul_args=B17, add_args=[L17])),
}

Case = namedtuple("Case", "name ea eb ec kw M N K variant limbs kernel")


def _mixed(name, tab, key, order, M, N, K, variant, ta=False):
    er, ez, ec, kw = tab[key]
    lr, lz = (1, int(key[-1])) if tab is UNEQUAL else (int(key[-1]),) * 2
    ea, eb, limbs = (er, ez, (lr, lz)) if order == "ra" else (ez, er, (lz, lr))
    if order == "rb":   # (the complex operand keeps the extent it doubles: rb swaps M and N)
        M, N = N, M
    return Case("rc_%s_%s_%s" % (key, order, name), ea, eb, ec, dict(kw, transposed_a=ta), M, N, K, variant, limbs, KERNEL_RC)


def _cplx(name, key, M, N, K, variant, ta=False):
    e, ec, kw = COMPLEX[key]
    return Case("cc_%s_%s" % (key, name), e, e, ec, dict(kw, transposed_a=ta), M, N, K, variant, (int(key[-1]),) * 2, KERNEL_CPLX)


def _cases():
    out = []
    # K crosses the k-tile with a ragged tail: 264 on 128-byte k-tiles, 200 on 64-byte ones.  QG_MFMA_PP at its smallest shape: the last
    # 256-wide tile of 1921 is 129 wide, and the oracle's bands over it (bands(), below) fit COST_CAP only with K <= 108, so that case
    # has one ragged k-tile, and a second one, whose last tiles are one row wide, has K = 264
    for order in ("ra", "rb"):
        out += [_mixed("64", LINEAR, "limb1", order, 130, 70, 264, 7),
                _mixed("128", LINEAR, "limb1", order, 1801, 641, 264, 8),
                _mixed("128bk64", LINEAR, "limb1", order, 2049, 1025, 200, 1),
                _mixed("pp", LINEAR, "limb1", order, 4097, 1921, 104, 9),
                _mixed("pp_k264", LINEAR, "limb1", order, 4097, 2049, 264, 9)]
        for key in ("limb2", "limb3"):
            out += [_mixed("64", LINEAR, key, order, 130, 70, 200, 6),
                    _mixed("128", LINEAR, key, order, 1801, 641, 200, 3),
                    _mixed("ppl", LINEAR, key, order, 2049, 1025, 200, 10)]
        for key in ("limb13", "limb12"):
            out.append(_mixed("128", UNEQUAL, key, order, 1801, 641, 200, 3))
    out += [_cplx("64", "limb1", 130, 70, 264, 7),
            _cplx("128", "limb1", 901, 641, 264, 8),
            _cplx("128bk64", "limb1", 1025, 1025, 200, 1),
            _cplx("pp", "limb1", 2049, 1921, 104, 9),
            _cplx("pp_k264", "limb1", 2049, 2049, 264, 9),
            _cplx("64", "limb2", 130, 70, 200, 6),
            _cplx("128", "limb2", 901, 641, 200, 3),
            _cplx("ppl", "limb2", 1025, 1025, 200, 10),
            _cplx("ppl_wide", "limb2", 2049, 1921, 200, 10),
            _cplx("ppl", "limb3", 1025, 1025, 200, 10)]
    # TransposedA, one per plan kind on a multi-tile 128 x 128 geometry
    out += [_mixed("128_ta", LINEAR, "limb1", "ra", 1801, 641, 264, 8, ta=True),
            _mixed("128_ta", LINEAR, "limb2", "rb", 1801, 641, 200, 3, ta=True),
            _cplx("128_ta", "limb2", 901, 641, 200, 3, ta=True)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the resident-path cases: one per stacked kernel on a multi-tile 128 x 128 geometry
RESIDENT = ["rc_limb13_ra_128", "cc_limb2_128"]
# the plane-mask cases' shapes: 64 x 64 tiles, and the two-group kernel whose 3 x 3 / 2 x 2 branch is taken on the device
MASK_SHAPES = [(130, 70, 200, 6), (2049, 1025, 200, 10)]


def desc(c: Case):
    return lower(c.ea, c.eb, c.ec, c.M, c.N, c.K, **c.kw)


def mask_desc(order, M, N, K):
    er, ez, ec, kw = MASK3
    if order == "rb":
        M, N = N, M
    return lower(*((er, ez) if order == "ra" else (ez, er)), ec, M, N, K, **kw)


def bands(extent, tile):
    """the index ranges [(lo, hi)] the oracle evaluates along one axis of C for tiles of `tile`: the first 8, the 8 around the first
    interior tile seam, and from 4 before the last tile's start to the end (merged where they touch)"""
    last = (extent - 1) // tile * tile
    raw = [(0, min(8, extent))]
    if tile < extent:
        raw.append((tile - 4, min(tile + 4, extent)))
    raw.append((max(last - 4, 0), extent))
    out = []
    for lo, hi in sorted(raw):
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(hi, out[-1][1]))
        else:
            out.append((lo, hi))
    return out


def blocks(M, N, tm, tn):
    """[(rows, cols)] of the oracle's work: each row band over every column, each column band over every row"""
    return [(r, (0, N)) for r in bands(M, tm)] + [((0, M), c) for c in bands(N, tn)]


def oracle_cost(kernel, M, N, K, tm, tn):
    """part-MACs of the oracle over blocks(): two real products per MAC of a mixed GEMM, four of a complex one"""
    return sum((r[1] - r[0]) * (c[1] - c[0]) for r, c in blocks(M, N, tm, tn)) * K * (2 if kernel == KERNEL_RC else 4)
