"""GPU parity of the register-counter tree kernels on trees of 13 to 16 levels (run with -m gpu on an MI355X).

The five tiled tree kernels (k_tree_fast, k_tree_pk16, k_tree_cplx, k_tree_cplx_pk16, k_tree64) are instantiated for at most 12
and at most 16 tree levels.  tests/test_gpu_parity.py stops at K = 4096 (12 levels): the 16-level instantiations — the upper four
slots of the binary counter's `up` array — are entered here.  K = 8192 is the smallest K with 13 levels; K = 4097 pads to the same
8192 leaves; K = 65536 (16 levels) parks in the last slot.  One descriptor per kernel and, for k_tree_fast and k_tree_cplx, one per
family of step forms, each against the oracle and against the general tree kernel (QG_OPT_GENERIC_TREE).  The planner gives every
form listed below at 13 and at 16 levels.  Bit-exact: integer work, no tolerance."""
import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qcomplex, Qu, RND, SAT, TRN, WRP, BasicComplexMul, TFComplexMul, lower
from test_gpu_parity import _vs_oracle, fields_equal

pytestmark = pytest.mark.gpu

E88 = Qu(8, 8)
E88Z = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
Q1516 = Qu(15, 16)
P = lambda i, f: Qu(i, f, True, RND.POS_INF, SAT.TCPL)
C5 = Qcomplex(P(6, 3), P(6, -3))
SMGN63 = Qu(6, 3, True, RND.NEG_INF, SAT.SMGN)

# (elements, C, lowering keywords, flags, kernel, the end of the planner's reason): descriptors of
# test_real_tree_kernel_step_forms, test_32_bit_word_tree_form and test_short_trees_on_the_register_counter_kernels
REAL = [
    (E88Z, E88Z, dict(), 0, "tree_i32", "one format, SAT::ZERO"),                                                       # QTF_ONE_ZERO
    (E88, Qu(12, 8), dict(add_args=[Qu(12, 8)]), 0, "tree_i32", "per-level formats, compact (clamps)"),                 # QTF_REC_CLAMP, split product
    (Qu(4, 3), Qu(8, 7), dict(mul_args=Qu(6, 7), add_args=[Qu(7, 7), Qu(8, 9, True, TRN.TCPL, WRP.TCPL)]), 0, "tree_i32",
     "per-level formats, compact"),                                                                                     # QTF_REC_BIASED, a wrapping level
    (E88, Qu(12, 8), dict(add_args=[Qu(12, 8, True, RND.CONV)], mul_args=Qu(10, 6, True, RND.CONV)), 0, "tree_i32",
     "per-level formats, compact (unbiased)"),                                                                          # QTF_REC_KINDS
    (E88, E88, dict(), 0, "tree_i32", "one format, SAT::TCPL, left-justified"),                                         # QTF_LJ
    (Qu(4, 3), Qu(4, 3), dict(), 0, "tree_i32", "one format, SAT::TCPL, left-justified, packed 16-bit"),                # QTF_PK16: k_tree_pk16
    (Qu(7, 8), Qu(7, 8), dict(), 0, "tree_i32", "one format, SAT::TCPL, left-justified, packed nodes"),                 # QTF_PK16_HYB16
    (Q1516, Q1516, dict(), 0, "tree_i32", "saturating word adds"),                                                      # QTF_WORD_MAD
    (E88, Qu(12, 8), dict(add_args=[Qu(12, 8)]), capi.OPT_RUNTIME_MODES, "tree_i32", "run-time modes"),                 # QTF_RUNTIME
    (Qu(15, 16), Qu(20, 12), dict(add_args=[Qu(24, 16)]), 0, "tree_i64", ""),                                           # k_tree64
]

# descriptors of test_complex_fixed_mode_step_forms
CPLX = [
    (C5, C5, dict(mul_args=TFComplexMul(ABT=Qu(7, 3, True, RND.POS_INF, SAT.TCPL))), 0, "fixed modes, compact"),        # QCF_COMPACT
    (Qcomplex(Qu(6, 3, True, RND.CONV), Qu(6, 3, True, RND.CONV)), Qcomplex(Qu(9, 3), Qu(9, 1)), dict(mul_args=TFComplexMul()), 0,
     "compact, branch-free rounding / overflow kinds"),                                                                 # QCF_KINDS_R
    (Qcomplex(Qu(5, 4, True, RND.INF, WRP.TCPL), Qu(6, 2, False, RND.ZERO, WRP.TCPL)), Qcomplex(Qu(6, 2, True, RND.INF, SAT.ZERO), Qu(5, 1, False, RND.CONV, WRP.TCPL)),
     dict(mul_args=TFComplexMul(), add_args=[Qcomplex(Qu(9, 3, True, RND.INF, WRP.TCPL), Qu(8, 1, False, TRN.SMGN, WRP.TCPL)),
                                             Qcomplex(Qu(7, 2, True, RND.ZERO, SAT.ZERO), Qu(9, 3, True, RND.CONV, SAT.SMGN))]), 0,
     "compact, rounding / overflow kinds"),                                                                             # QCF_KINDS
    (Qcomplex(P(8, 4), P(8, 4)), C5, dict(mul_args=TFComplexMul()), 0, "fixed modes, one clamp, left-justified"),       # QCF_LJ
    (Qcomplex(SMGN63, SMGN63), C5, dict(mul_args=BasicComplexMul()), 0, "fixed modes, one clamp for the whole loop"),   # QCF_UNIFORM
    (C5, C5, dict(mul_args=TFComplexMul()), 0, "fixed modes, one clamp, packed 16-bit"),                                # QCF_PK16: k_tree_cplx_pk16
    (C5, C5, dict(mul_args=BasicComplexMul()), capi.OPT_RUNTIME_MODES, "run-time modes"),                               # QCF_RUNTIME
]


def _case(oracle, ea, ec, kw, flags, kernel, form, M, N, K, generic):
    d = lower(ea, ea, ec, M, N, K, **kw)
    info = capi.classify(d, flags)
    assert capi.KERNEL_NAMES[info.kernel] == kernel and info.reason.decode().endswith(form), (info.reason, form)
    a = _vs_oracle(oracle, ea, ea, ec, M, N, K, flags=flags, expect_kernel=kernel, **kw)
    b = _vs_oracle(oracle, ea, ea, ec, M, N, K, flags=capi.OPT_GENERIC_TREE, expect_kernel=generic, **kw)
    assert fields_equal(a, b)


@pytest.mark.parametrize("case", REAL, ids=lambda c: (c[5] or c[4]).replace(" ", "_"))
def test_13_level_trees_real(oracle, case):
    """M = 70, N = 41: two row tiles of the 64-row kernels, both partial in N."""
    ea, ec, kw, flags, kernel, form = case
    _case(oracle, ea, ec, kw, flags, kernel, form, 70, 41, 8192, "tree_i64")


@pytest.mark.parametrize("case", CPLX, ids=lambda c: c[4].replace(" ", "_"))
def test_13_level_trees_complex(oracle, case):
    e, ec, kw, flags, form = case
    _case(oracle, e, ec, kw, flags, "tree_cplx_i32", form, 33, 29, 8192, "tree_cplx")


def test_13_level_trees_padded_k(oracle):
    """K = 4097: the same 8192 leaves, the upper 4095 of them the packed operands' zero padding."""
    ea, ec, kw, flags, kernel, form = REAL[1]
    _case(oracle, ea, ec, kw, flags, kernel, form, 70, 41, 4097, "tree_i64")
    e, ec, kw, flags, form = CPLX[0]
    _case(oracle, e, ec, kw, flags, "tree_cplx_i32", form, 33, 29, 4097, "tree_cplx")


def test_16_level_trees(oracle):
    """K = 65536: the counter carries through the last slot of `up`."""
    ea, ec, kw, flags, kernel, form = REAL[0]
    _case(oracle, ea, ec, kw, flags, kernel, form, 5, 3, 65536, "tree_i64")
    e, ec, kw, flags, form = CPLX[0]
    _case(oracle, e, ec, kw, flags, "tree_cplx_i32", form, 5, 3, 65536, "tree_cplx")
