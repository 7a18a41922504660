"""Three-digit Karatsuba on unsigned base-64 digits (qg_mfma_k6.hip), restated in numpy: six digit products recombine to the plain
integer dot product, the byte-wise digit sums never carry, the bias / row-sum correction gives back the signed product, and each of
the six int32 sums stays below 2^31 up to the planner's bound.  Then the planner: which descriptors take the form.  CPU only."""
import numpy as np
import pytest

from qublas_amd import capi
from qublas_amd.desc import Qu, SAT, TRN, Tags, lower

E88 = Qu(8, 8, True, TRN.TCPL, SAT.ZERO)
KW88 = dict(mul_args=Tags(17, 16), add_args=[Qu(33, 16)])
K6 = b"six products"


def digits(x):
    """unsigned base-64 digits of non-negative x < 2^18"""
    assert x.min() >= 0 and x.max() < (1 << 18)
    return [(x >> (6 * l)) & 63 for l in range(3)]


def k6_dot(a, b, bias_a, bias_b):
    """sum_k a[i,k] b[k,j] the way the kernel forms it: int32 accumulators, 64-bit recombination, row-sum correction"""
    K = a.shape[1]
    d, e = digits(a + bias_a), digits(b + bias_b)
    for x in d + e:
        assert x.max() <= 63
    for s in (d[0] + d[1], d[1] + d[2], d[0] + d[2], e[0] + e[1], e[1] + e[2], e[0] + e[2]):
        assert s.max() <= 126                     # a valid int8, and four of them add in one 32-bit add without a carry
    p = lambda x, y: x.astype(np.int64) @ y.astype(np.int64)
    S00, S11, S22 = p(d[0], e[0]), p(d[1], e[1]), p(d[2], e[2])
    P01, P12, P02 = p(d[0] + d[1], e[0] + e[1]), p(d[1] + d[2], e[1] + e[2]), p(d[0] + d[2], e[0] + e[2])
    for acc in (S00, S11, S22, P01, P12, P02):
        assert acc.min() >= 0 and acc.max() < (1 << 31)       # ONE product per int32 accumulator
    x = S00 + 64 * (P01 - S00 - S11) + 64 ** 2 * (P02 - S00 - S22 + S11) + 64 ** 3 * (P12 - S11 - S22) + 64 ** 4 * S22
    rs_a = (a + bias_a).astype(np.int64).sum(axis=1)
    rs_b = (b + bias_b).astype(np.int64).sum(axis=0)
    return x - bias_b * rs_a[:, None] - bias_a * rs_b[None, :] + K * bias_a * bias_b


def test_packed_bytes_add_without_carry():
    """the kernel's v_add_u32 on four packed digits: the 32-bit sum of two registers is the byte-wise sum"""
    rng = np.random.default_rng(1)
    x, y = rng.integers(0, 64, (1000, 4), dtype=np.uint32), rng.integers(0, 64, (1000, 4), dtype=np.uint32)
    x[0], y[0] = 63, 63
    pack = lambda v: v[:, 0] | (v[:, 1] << 8) | (v[:, 2] << 16) | (v[:, 3] << 24)
    s = (pack(x) + pack(y)).astype(np.uint32)
    assert np.array_equal(s, pack(x + y)) and (x + y).max() <= 126
    z = rng.integers(0, 64, (1000, 4), dtype=np.uint32)       # (d1 + d2) + d0 - d2: at most 189 in a byte on the way
    assert np.array_equal((pack(x) + pack(y) + pack(z) - pack(y)).astype(np.uint32), pack(x + z))


@pytest.mark.parametrize("wa,sa,wb,sb", [(16, 1, 16, 1), (17, 1, 17, 1), (17, 0, 17, 0), (18, 0, 18, 0), (17, 1, 17, 0), (12, 1, 17, 1)])
def test_recombination_on_random_and_extreme_operands(wa, sa, wb, sb):
    """W value bits, S sign: signed formats are biased by 2^W into [0, 2^(W+1))"""
    rng = np.random.default_rng(wa * 100 + wb)
    lo_a, hi_a = (-(1 << wa) if sa else 0), (1 << wa) - 1
    lo_b, hi_b = (-(1 << wb) if sb else 0), (1 << wb) - 1
    bias_a, bias_b = (1 << wa if sa else 0), (1 << wb if sb else 0)
    M, N, K = 24, 20, 333
    cases = [(rng.integers(lo_a, hi_a + 1, (M, K)), rng.integers(lo_b, hi_b + 1, (K, N)))]
    edge_a = np.array([lo_a, lo_a + 1, -1 if sa else 0, 0, 1, hi_a - 1, hi_a])
    edge_b = np.array([lo_b, lo_b + 1, -1 if sb else 0, 0, 1, hi_b - 1, hi_b])
    cases.append((rng.choice(edge_a, (M, K)), rng.choice(edge_b, (K, N))))
    for va in (lo_a, hi_a):
        for vb in (lo_b, hi_b):
            cases.append((np.full((M, K), va), np.full((K, N), vb)))
    for a, b in cases:
        a, b = a.astype(np.int64), b.astype(np.int64)
        assert np.array_equal(k6_dot(a, b, bias_a, bias_b), a @ b)


def test_accumulators_at_the_planner_bound():
    """every digit at 63: P01 = K * 126^2, inside int32 exactly while K * 126^2 < 2^31"""
    kmax = ((1 << 31) - 1) // (126 * 126)
    assert kmax == 135266 and kmax * 126 * 126 < (1 << 31) <= (kmax + 1) * 126 * 126
    a = np.full((2, kmax), (1 << 18) - 1, dtype=np.int64)
    b = np.full((kmax, 2), (1 << 18) - 1, dtype=np.int64)
    assert np.array_equal(k6_dot(a, b, 0, 0), a @ b)


def reason(M, N, K, flags=0, e=E88, c=Qu(23, 8), kw=KW88):
    info = capi.classify(lower(e, e, c, M, N, K, **kw), flags)
    assert capi.KERNEL_NAMES[info.kernel] == "mfma_i8_limb" and list(info.limbs)[:2] == [3, 3]
    return bytes(info.reason)


def test_planner_eligibility():
    # the largest reduction length of a single-launch 3 x 3 plan is 43 690 (3 K <= 2^17 - 1: the schoolbook layout's own bound, which
    # decides whether the plan is composite); the form's bound K * 126^2 < 2^31 (K <= 135 266) lies beyond it, so the form ends where
    # the k-chunked composite plans begin, and those keep the balanced limbs
    assert K6 in reason(2048, 2048, 43690)
    over = reason(2048, 2048, 43691)
    assert K6 not in over and b"k-chunk" in over
    wide = dict(mul_args=Tags(17, 16), add_args=[Qu(36, 16)])
    for k in (135266, 135267):          # just below and just above K * 126^2 < 2^31: k-chunked composite plans on either side today
        r = reason(2048, 2048, k, kw=wide)
        assert K6 not in r and b"k-chunk" in r
    # the switch, the lock-step flag, and shapes below a tile per CU
    assert K6 in reason(4096, 4096, 4096)
    assert b"nine products" in reason(4096, 4096, 4096, capi.OPT_SCHOOLBOOK_LIMBS)
    assert K6 not in reason(4096, 4096, 4096, capi.OPT_LOCKSTEP_TILES)
    assert K6 not in reason(1024, 1024, 4096)
    # narrow C (2-byte container) and 19-bit operands keep the nine products
    assert K6 not in reason(2048, 2048, 512, c=Qu(7, 8))
    e19 = Qu(10, 8)
    assert b"nine products" in reason(2048, 2048, 512, e=e19, c=Qu(25, 8), kw=dict(mul_args=Tags(21, 16), add_args=[Qu(33, 16)]))


def test_packed_geometry_of_the_form():
    """A on 96-row tiles, B on 128-row tiles, three planes + trailer + int64 row sums; packed C on the 128 x 128 tiles of every limb plan"""
    info = capi.classify(lower(E88, E88, Qu(23, 8), 4096, 4096, 4096, **KW88))
    mp, np_, kp = 43 * 96, 4096, 4096
    assert list(info.packed_bytes)[:3] == [3 * mp * kp + 256 + 8 * mp, 3 * np_ * kp + 256 + 8 * np_, 4096 * np_ * 4]
