"""The case table of the linear class's conversion sites — TEST INFRASTRUCTURE, not a test module.

In the linear class rounding and overflow happen once, in the conversion sum -> C, and that conversion is written out in every kernel's
epilogue and in the conversion passes ("The conversion sites of the linear class").  SITES names, per site, the operands, the
shape, the flags and the geometry it must reach (QMfmaCfg::variant, limb counts, centred or Karatsuba layout, composite groups and
k-chunks); every site crosses the C formats of its containers (formats(), below), and each (site, format) pair is one Case with the
wide_ep, launches and container it must reach (expected()).  tests/test_linear_c_coverage.py pins all of that through the planner driver
on the CPU and checks the witnesses and shares of the designed sums (tests/designed_sums.py); tests/test_gpu_linear_c.py runs every case
on the GPU.  STACKED_CASES (at the end) are the complex x complex and complex x real plans, whose second passes convert each part of C by
its own format.

Shapes: M and N end in a ragged tile of 9 rows and 13 columns (at least 9 wide, no multiple of 4, and at least as wide as the longest
offset list); K is just above one k-tile with a ragged tail, or as long as the designed sums need; the persistent kernels get 17 x 16,
17 x 17 or 22 x 17 tiles, a partly filled second round."""
from collections import namedtuple

import designed_sums as DS
from qublas_amd import capi
from qublas_amd.desc import Qu, RND, SAT, TRN, WRP, Tags, lower

# QMfmaCfg::variant -> (enumerator, BK, TM, TN) (qublas_amd/csrc/qg_geom.h)
VARIANTS = {1: ("QG_MFMA_128", 64, 128, 128), 2: ("QG_MFMA_256", 64, 256, 256), 3: ("QG_MFMA_LIMB_128", 64, 128, 128), 6: ("QG_MFMA_LIMB_64", 64, 64, 64),
            7: ("QG_MFMA_64_BK128", 128, 64, 64), 8: ("QG_MFMA_128_BK128", 128, 128, 128), 9: ("QG_MFMA_PP", 128, 256, 256),
            10: ("QG_MFMA_PPL", 64, 128, 128), 11: ("QG_MFMA_K6", 64, 96, 128), 12: ("QG_MFMA_RING", 64, 128, 128)}
PERSISTENT = {9, 10, 11}
COST_CAP = 1.5e8   # part-MACs of oracle work per test (tests/stacked_cases.py)

# ---- C formats.  (d, signed, QuMode, OfMode): all seven QuModes and all four OfModes in rotation; TRN::TCPL + SAT::TCPL with d >= 1 (the
# shift-and-clamp epilogue, FAST where a kernel has it) and its two neighbours across qg_step_is_shift_clamp; d = 1 (half = 1); one deep
# shift; d = 0; one left shift; unsigned C fed by signed sums
DEEP = "deep"
MODES = [
    (3, True, TRN.TCPL, SAT.TCPL),
    (3, True, TRN.TCPL, SAT.ZERO),
    (3, True, RND.POS_INF, SAT.TCPL),
    (1, True, RND.NEG_INF, SAT.SMGN),
    (DEEP, True, RND.CONV, WRP.TCPL),
    (0, True, RND.ZERO, SAT.ZERO),
    (-1, True, RND.INF, WRP.TCPL),
    (3, False, TRN.SMGN, WRP.TCPL),
    (2, True, RND.INF, SAT.SMGN),
    (4, False, RND.ZERO, SAT.TCPL),
    (2, True, RND.CONV, SAT.TCPL),
]
# value bits per container: the smallest W of the container (its bounds are then the nearest a short K can reach), 7 for one byte
CONTAINER_W = {1: 7, 2: 8, 4: 16, 8: 32}
# the longest centre segment a bound-reaching case may need: K stays a few k-tiles, inside what the single-launch linear plans admit for the
# sites' level types (an int<4,3> plan on Qu<21,6> levels leaves the MFMA kernels for the tree class near K = 5200, the length a 16-bit C
# shifted by 8 would need); beyond it the deep shift runs on a roomy C
MAX_DIGITS = 256


def fmt(Fs, W, d, signed, Q, O):
    return Qu(W - (Fs - d), Fs - d, signed, Q, O)


def formats(Fs, container, deep, W=None):
    """the C formats of one container for sums of Fs fraction bits; `deep` is the deep shift (8 where K can reach the bounds then); W: the
    value bits where not the container's smallest"""
    W = W or CONTAINER_W[container]
    # (an unsigned WRP::TCPL C of exactly 32 value bits is refused: the reference's multi-word artefact; 33 there)
    return [fmt(Fs, W + (W == 32 and not s and O == WRP.TCPL), deep if d == DEEP else d, s, Q, O) for d, s, Q, O in MODES]


def wide_formats(Fs):
    """C of 32 and more value bits whose bounds a short K cannot reach under a right shift: the left shifts reach them (every OfMode,
    both signs), and the right shifts run every QuMode on a roomy C, where the ties are what the data can hit.  Single-limb plans take
    these through the 64-bit conversion pass (wide_ep): C above 30 value bits, or a left shift that takes the sums beyond 31 bits"""
    left = [fmt(Fs, 32, -24, True, TRN.TCPL, SAT.TCPL), fmt(Fs, 32, -22, True, RND.CONV, SAT.ZERO), fmt(Fs, 33, -23, True, TRN.TCPL, SAT.SMGN),
            fmt(Fs, 32, -25, True, RND.INF, WRP.TCPL), fmt(Fs, 33, -24, False, TRN.SMGN, WRP.TCPL), fmt(Fs, 34, -26, False, TRN.TCPL, SAT.TCPL),
            fmt(Fs, 30, -12, True, TRN.TCPL, SAT.TCPL),    # 30 value bits, and a left shift that takes the sums beyond 31 bits
            fmt(Fs, 31, -20, True, TRN.TCPL, SAT.ZERO)]    # 31 value bits: a 4-byte container, and the pass all the same
    roomy = [fmt(Fs, 40, d, True, Q, SAT.TCPL) for d, Q in ((3, TRN.TCPL), (3, TRN.SMGN), (2, RND.POS_INF), (1, RND.NEG_INF), (4, RND.ZERO), (3, RND.INF), (8, RND.CONV), (0, TRN.TCPL))]
    return left, roomy


def I(bits):
    """plain C integer of `bits` bits, wrapping: a ring type"""
    return Qu(bits - 1, 0, True, TRN.TCPL, WRP.TCPL)


# ---- operands.  name: (A, B, mul tags, exact sum format)
E43, E65, E77, E88, E108 = Qu(4, 3), Qu(6, 5), Qu(7, 7), Qu(8, 8, True, TRN.TCPL, SAT.ZERO), Qu(10, 8)
U8, Q78, E1212, Q1516 = Qu(8, 0, False), Qu(7, 8), Qu(12, 12), Qu(15, 16)
OPERANDS = {
    "e43": (E43, E43, Tags(9, 6), Qu(21, 6)),               # 8 bits: one limb
    "e43k": (E43, E43, Tags(9, 6), Qu(27, 6)),              # ... with levels that hold K = 131 077: two k-chunks
    "e65": (E65, E65, Tags(13, 10), Qu(28, 10)),            # 12 bits with the sign: two limbs, Karatsuba-eligible
    "e77": (E77, E77, Tags(15, 14), Qu(28, 14)),            # 15 bits: two limbs, schoolbook (not Karatsuba-eligible, nothing to centre)
    "e88": (E88, E88, Tags(17, 16), Qu(29, 16)),            # 17 bits: three limbs; three base-64 digits on the six-product kernel
    "e108": (E108, E108, Tags(21, 16), Qu(33, 16)),         # 19 bits: three limbs, nine products
    "u8": (U8, U8, Tags(16, 0, False), Qu(30, 0, False)),   # uint8: centred onto one limb
    "q78": (Q78, Q78, Tags(15, 16), Qu(28, 16)),            # 16 bits: centred onto two limbs
    "e1212": (E1212, E1212, Tags(25, 24), Qu(37, 24)),      # 25 bits: 2 x 2 groups of two limbs
    "q1516": (Q1516, Q1516, Tags(31, 32), Qu(43, 32)),      # 32 bits: 2 x 2 groups, sums of more than 64 bits (the 128-bit combine)
    # ring plans (wrapping level types): the conversion after the ring wrap; the designed sums stay inside the ring
    "ring1": (I(8), I(8), Tags.of(I(16)), I(16)),           # int8 into an int16 ring: one limb product
    "ring3": (I(8), I(16), Tags.of(I(24)), I(24)),          # int8 x int16 into an int24 ring: three
    "ring10": (I(32), I(32), Tags.of(I(32)), I(32)),        # int32 ring: ten
}

Site = namedtuple("Site", "name op M N K0 flags variant limbs centred digit6 comp containers second")
Case = namedtuple("Case", "name site ec container roomy ta idx extra")


def _site(name, op, M, N, K0, variant, limbs, containers, *, flags=0, centred=False, digit6=False, comp=None, second=()):
    return Site(name, op, M, N, K0, flags, variant, limbs, centred, digit6, comp, containers, tuple(second))


SMALL, RING, MID, MANY, HUGE = (137, 77), (265, 141), (1801, 1165), (2057, 2061), (4105, 3853)
SITES = [
    # k_mfma, single limb: 64x64 x 128, 128x128 x 128, 128x128 x 64; the second kernel of the small shape is the tree class
    _site("k64", "e43", *SMALL, 135, 7, (1, 1), (1, 2, 4), second=[capi.OPT_FORCE_TREE]),
    # ... a 4-byte C shifted by 8 with its bounds among the sums needs K = 5200 of these operands: on levels that hold such sums
    _site("k64_deep", "e43k", *SMALL, 135, 7, (1, 1), ("deep4",), second=[capi.OPT_FORCE_TREE]),
    _site("k128", "e43", *MID, 135, 8, (1, 1), (1, 2, 4)),
    _site("k128bk64", "e43", *MANY, 71, 1, (1, 1), (1, 2, 4)),
    # k_mfma16, 256x256 lock-step, and k_mfma_pp on the same descriptors: 17 x 16 tiles
    _site("k256", "e43", *HUGE, 71, 2, (1, 1), (1, 2, 4), flags=capi.OPT_LOCKSTEP_TILES),
    _site("pp", "e43", *HUGE, 135, 9, (1, 1), (1, 2, 4)),
    # the 64-bit conversion pass behind k_mfma and behind k_mfma_pp (container 8 hands raw sums to it)
    _site("wide64", "e43", *SMALL, 135, 7, (1, 1), ("wide",)),
    _site("wide_pp", "e43", *HUGE, 135, 9, (1, 1), ("wide",)),
    # k_mfma, limbs: the run-time container switch of qg_step_all<int64>; 64x64 and the row-step 128x128 form
    _site("limb64_22", "e77", *SMALL, 71, 6, (2, 2), (1, 2, 4, "wide"), second=[capi.OPT_FORCE_TREE]),
    _site("limb64_33", "e88", *SMALL, 71, 6, (3, 3), (1, 2, 4, 8, "pieces"), second=[capi.OPT_FORCE_TREE]),
    _site("limb128_22", "e77", *MID, 71, 3, (2, 2), (1, 2, 4, "wide")),
    _site("limb128_33", "e88", *MID, 71, 3, (3, 3), (1, 2, 4, 8, "pieces")),
    _site("kara", "e65", *MID, 71, 3, (2, 2), (1, 2, 4, "wide"), digit6=True),
    # centred operands on the lock-step body (uint8: the 64-bit qg_step branch; Q7.8: two limbs) and in k_mfma_pp (convert16c)
    _site("cent_u8", "u8", *SMALL, 135, 7, (1, 1), (1, 2, 4), centred=True, second=[capi.OPT_BALANCED_LIMBS]),
    _site("cent_u8_128", "u8", *MID, 135, 8, (1, 1), (1, 2, 4), centred=True),
    _site("cent_q78", "q78", *MID, 71, 3, (2, 2), (1, 2, 4, 8), centred=True, second=[capi.OPT_BALANCED_LIMBS]),
    _site("pp_cent_u8", "u8", *HUGE, 135, 9, (1, 1), (1, 2, 4), centred=True),
    # the two-group limb kernels and the six-product kernel: containers 4 and 8 (narrower C runs QG_MFMA_LIMB_128)
    _site("ppl33", "e108", *MANY, 71, 10, (3, 3), (4, 8, "pieces")),
    _site("ppl22", "e77", *MANY, 71, 10, (2, 2), (4, "wide")),
    _site("k6", "e88", *MANY, 71, 11, (3, 3), (4, 8, "pieces"), digit6=True),
    _site("k6_schoolbook", "e88", *MANY, 71, 10, (3, 3), (4, 8), flags=capi.OPT_SCHOOLBOOK_LIMBS),
    # k_mfma_ring: C differs from the ring type, so the step after the wrap is not skipped
    _site("ring1", "ring1", *RING, 71, 12, (1, 1), (1, 2)),
    _site("ring3", "ring3", *RING, 71, 12, (1, 3), (1, 2)),
    _site("ring10", "ring10", *RING, 71, 12, (4, 4), (1, 2, 4)),
    # k_lin_combine: k-chunks of a single limb; 2 x 2 groups of two limbs; sums of more than 64 bits.  comp: (A groups, B groups, k-chunks)
    _site("comb_k", "e43k", 25, 29, 131077, 8, (1, 1), (2, 4), comp=(1, 1, 2)),
    _site("comb_g", "e1212", *SMALL, 71, 6, (4, 4), (1, 2, 4, 8), comp=(2, 2, 1)),
    _site("comb_w", "q1516", *SMALL, 71, 6, (4, 4), (4, 8, "huge"), comp=(2, 2, 1), centred=True),
]
BY_SITE = {s.name: s for s in SITES}
assert len(BY_SITE) == len(SITES)


def _deep(s, c):
    """8 where the bounds of a C shifted by 8 are within MAX_DIGITS reduction indices and inside the sum format, else 3"""
    ea, eb, _, es = OPERANDS[s.op]
    far = 5 << (CONTAINER_W[c] + 8)
    return 8 if far <= min(MAX_DIGITS * ea.raw_max * eb.raw_max, es.raw_max) else 3


def _cases():
    out = []
    for s in SITES:
        es = OPERANDS[s.op][3]
        Fs = es.fracBits
        for c in s.containers:
            extra = ()
            if c == "wide":
                left, roomy = wide_formats(Fs)
                fs = [(f, False) for f in left] + [(f, True) for f in roomy]
            elif c == "pieces":
                # three limbs / three digits, a roomy 8-byte C: centres at the piece boundaries of the recombinations (k6_recombine's
                # 32-bit pieces, the x * 256 + acc[w] chain), as far as K reaches
                fs = [(fmt(Fs, 50, 2, True, RND.CONV, SAT.TCPL), True)]
                extra = [m * (1 << 32) - e for m in (1, -1, 2, 3, -5, 40) for e in (0, 1)] + [m << (24 + n) for m in (1, -1, 3) for n in (0, 8, 14)]
            elif c == "deep4":
                fs = [(fmt(Fs, CONTAINER_W[4], 8, True, Q, O), False) for Q, O in ((RND.CONV, WRP.TCPL), (RND.POS_INF, SAT.SMGN))]
            elif c == "huge":
                # sums beyond 64 bits into a roomy C behind a long right shift
                fs = [(fmt(Fs, 40, 36, True, RND.INF, SAT.TCPL), True), (fmt(Fs, 44, 33, True, RND.ZERO, SAT.TCPL), True)]
            else:
                fs = [(f, False) for f in formats(Fs, c, _deep(s, c))]
                if _deep(s, c) != 8:
                    # the bounds behind a shift of 8 are out of reach: the deep shift on a roomy C of the same container, whose ties
                    # (both signs, even and odd kept part) and neighbours of half the data does hit
                    fs.append((fmt(Fs, CONTAINER_W[c], 8, True, RND.CONV, SAT.TCPL), True))
            for n, (f, roomy) in enumerate(fs):
                if es.W > 63 and f.QuMode == RND.CONV:
                    # (RND::CONV of a sum wider than 64 bits is refused: a multi-word artefact of the reference)
                    f = Qu(f.intBits, f.fracBits, f.isSigned, RND.POS_INF, f.OfMode)
                out.append(Case("%s-c%s-%02d" % (s.name, c, n), s.name, f, c, roomy, n % 4 == 3, len(out), tuple(extra)))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def is_fast(es, ec):
    """qg_step_is_shift_clamp: the compile-time FAST epilogue of the two-group kernels"""
    return ec.QuMode == TRN.TCPL and ec.OfMode == SAT.TCPL and es.fracBits - ec.fracBits >= 0


def pow2_bytes(bits):
    b = 1
    while 8 * b < bits:
        b *= 2
    return b


# the format the planner gives to a composite of one chunk and one group although its site runs one launch: the longest left shift (26
# bits into an unsigned C of 34 value bits) of the 15-bit two-limb operands' sums, which the kernels' 64-bit step would not hold (the
# rule: qg_geom.cpp, linear_kernel).  (operands, signed, shift, value bits of C)
ONE_CHUNK_COMPOSITE = ("e77", False, -26, 34)


def expected(c: Case):
    """{wide_ep, launches, container, comp}: what the planner must answer for the case beyond its site's geometry"""
    s = BY_SITE[c.site]
    es = OPERANDS[s.op][3]
    comp = s.comp
    # a centred single-limb plan whose C shifts left runs as a composite of one chunk and one group: its combine pass converts
    if s.centred and s.limbs == (1, 1) and es.fracBits < c.ec.fracBits and not comp:
        comp = (1, 1, 1)
    if (s.op, c.ec.isSigned, es.fracBits - c.ec.fracBits, c.ec.W) == ONE_CHUNK_COMPOSITE:
        comp = (1, 1, 1)
    wide = int(s.limbs == (1, 1) and not comp and s.variant != 12 and c.container == "wide")
    launches = comp[2] * (comp[0] * comp[1] + 1) if comp else 1 + wide
    return dict(wide_ep=wide, launches=launches, container=pow2_bytes(c.ec.storage_bits), comp=comp)


def band_blocks(M, N, TM, TN):
    """[(rows, cols)] the oracle evaluates: the row bands of stacked_cases.bands() over every column, and its column bands over the rows
    the row bands left out"""
    import stacked_cases as S
    rb = S.bands(M, TM)
    out = [(r, (0, N)) for r in rb]
    gaps = [(a[1], b[0]) for a, b in zip([(0, 0)] + rb, rb + [(M, M)]) if a[1] < b[0]]
    return out + [(g, c) for c in S.bands(N, TN) for g in gaps]


def oracle_cost(M, N, K, TM, TN):
    """MACs of the oracle over band_blocks()"""
    return sum((r[1] - r[0]) * (c[1] - c[0]) for r, c in band_blocks(M, N, TM, TN)) * K


def plan(c: Case):
    """(site, operand formats (ea, eb, es), centres, offsets, K): what the case's designed sums are made of"""
    s = BY_SITE[c.site]
    ea, eb, _, es = OPERANDS[s.op]
    signed = ea.isSigned
    offsets = DS.default_offsets(es, c.ec, signed)
    # a roomy C: nothing near the bounds is within reach, the centres spread over what the site's base K gives
    reach = min((min(s.K0, MAX_DIGITS) - 8) * eb.raw_max * ea.raw_max // 2, es.raw_max // 2) if c.roomy else None
    centres = DS.default_centres(es, c.ec, len(offsets), signed, extra=[e for e in c.extra if reach is None or abs(e) <= reach], reach=reach)
    BK = VARIANTS[s.variant][1]
    K = max(s.K0, DS.k_needed(ea, eb, centres, offsets))
    if K % BK == 0:
        K += 7
    return s, (ea, eb, es), centres, offsets, K


def desc(c: Case, K=None):
    s, (ea, eb, es), _, _, k = plan(c)
    return lower(ea, eb, c.ec, s.M, s.N, K or k, mul_args=OPERANDS[s.op][2], add_args=[es], transposed_a=c.ta)


def designed(oracle, c: Case):
    """(descriptor, Designed) of a case; the phase (ri, rj) rotates with the case"""
    s, (ea, eb, es), centres, offsets, K = plan(c)
    dz = DS.build(oracle, ea, eb, es, s.M, s.N, K, centres, offsets, ri=(3 * c.idx) % len(centres), rj=(5 * c.idx) % len(offsets), transposed_a=c.ta)
    return desc(c, K), dz


# ---- the stacked plans: complex x complex (mfma_cplx, k_cplx_combine) and complex x real (mfma_rc, k_rc_convert), plain and as members
# of a stacked block-diagonal batch (QG_OPT_BATCHED_STACKED, k_stack_combine_bd).  One real limb GEMM on the stacked operand hands raw
# 64-bit dot products to a second pass, which converts each part of C by its own format.  B's imaginary part is zero (complex x complex)
# or B is the real operand, so C_re = A_re . B_re and C_im = A_im . B_re: A's parts carry two independent centre lists, the offset
# segment is shared (the union of what both parts' shifts need), and the parts of C take different modes.
KERNEL_CPLX, KERNEL_RC = 7, 12   # QG_KERNEL_MFMA_CPLX, QG_KERNEL_MFMA_RC (include/qgemul.h)
STACKED_SHAPE = (137, 93)        # ragged last tiles of 9 rows and 29 columns: the united offset list has up to 29 entries
StackedCase = namedtuple("StackedCase", "name kind ec container roomy ta idx")


def stacked_operands(kind):
    """(A, B, lowering keywords, sum formats) of a kind: the single-limb elements of tests/stacked_cases.py"""
    import stacked_cases as S
    if kind == "cc":
        e, _, kw = S.COMPLEX["limb1"]
        return e, e, kw, kw["add_args"][0]
    er, ez, _, kw = S.LINEAR["limb1"]
    return ez, er, kw, kw["add_args"][0]


def _stacked_cases():
    from qublas_amd.desc import Qcomplex
    out = []
    for kind in ("cc", "rc"):
        es = stacked_operands(kind)[3]
        for c in (2, 4):
            per_part = []
            for p, f in enumerate((es.real, es.imag)):
                deep = 8 if c == 2 else 3
                # (the mixed element's imaginary part has 5 bits: its sums reach the bounds of a 12-bit C part, not of a 16-bit one,
                # before they leave the level type; the real part's 17 storage bits make the container)
                W = 12 if (kind, c, p) == ("rc", 4, 1) else CONTAINER_W[c]
                fs = [(x, False) for x in formats(f.fracBits, c, deep, W)]
                if deep != 8:
                    fs.append((fmt(f.fracBits, W, 8, True, RND.CONV, SAT.TCPL), True))
                per_part.append(fs)
            n_f = len(per_part[0])
            for n in range(n_f):
                (f_re, roomy_re), (f_im, roomy_im) = per_part[0][n], per_part[1][(n + 4) % n_f]   # the parts of C take different modes
                out.append(StackedCase("%s-c%d-%02d" % (kind, c, n), kind, Qcomplex(f_re, f_im), c, (roomy_re, roomy_im), n % 4 == 3, len(out)))
    return out


STACKED_CASES = _stacked_cases()
STACKED_BY_NAME = {c.name: c for c in STACKED_CASES}


def _pad_to(xs, n, unit):
    xs, k = list(xs), 4
    while len(xs) < n:
        for v in (k * unit, -k * unit):
            if v not in xs and len(xs) < n:
                xs.append(v)
        k += 1
    return xs


def stacked_plan(c: StackedCase):
    """(ea, eb, kw, es, centres of the real parts, centres of the imaginary parts, united offsets, K)"""
    ea, eb, kw, es = stacked_operands(c.kind)
    parts = ((ea.real, es.real, c.ec.real, c.roomy[0]), (ea.imag, es.imag, c.ec.imag, c.roomy[1]))
    br = eb.real if hasattr(eb, "real") else eb
    offsets = []
    for _, sp, cp, _ in parts:
        offsets += [o for o in DS.default_offsets(sp, cp) if o not in offsets]
    k = 2
    while len(offsets) % 2 == 0 or any(t % len(offsets) == 0 for t in DS.TILE_EXTENTS):
        offsets += [v for v in (max(offsets) + k,) if v not in offsets]
        k += 1
    assert len(offsets) <= STACKED_SHAPE[1] % 64
    lists = []
    for pa, sp, cp, roomy in parts:
        reach = min(120 * br.raw_max * pa.raw_max // 2, sp.raw_max // 2) if roomy else None
        lists.append(DS.default_centres(sp, cp, len(offsets), reach=reach))
    P = max(len(x) for x in lists)
    while not DS.well_formed(P, len(offsets)):
        P += 2
    lists = [_pad_to(x, P, DS.geometry(sp, cp)[1]) for x, (_, sp, cp, _) in zip(lists, parts)]
    need = [DS.segments(pa, br, x, offsets) for x, (pa, _, _, _) in zip(lists, parts)]
    K = max(135, sum(max(a, b) for a, b in zip(*need)))
    if K % 128 == 0:
        K += 7
    return ea, eb, kw, es, lists[0], lists[1], offsets, K


def stacked_desc(c: StackedCase):
    ea, eb, kw, _, _, _, _, K = stacked_plan(c)
    return lower(ea, eb, c.ec, *STACKED_SHAPE, K, transposed_a=c.ta, **kw)


def stacked_designed(oracle, c: StackedCase, member=0):
    """(descriptor, A, B, Designed of the real parts, Designed of the imaginary parts); `member` shifts the phase"""
    ea, eb, kw, es, cr, ci, offsets, K = stacked_plan(c)
    M, N = STACKED_SHAPE
    A, B, dr, di = DS.build_stacked(oracle, ea, eb, es, M, N, K, cr, ci, offsets, ri=(3 * c.idx + 5 * member) % len(cr),
                                    rj=(5 * c.idx + 3 * member) % len(offsets), transposed_a=c.ta)
    return stacked_desc(c), A, B, dr, di
