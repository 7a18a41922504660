"""Operands with a PRESCRIBED exact dot product per output element — TEST INFRASTRUCTURE, not a test module.

In the linear class the engine holds the dot product exactly; rounding and overflow happen once, in the conversion sum -> C of each
kernel's epilogue.  build() makes host-layout A and B whose exact raw dot product is

    s(i, j) = centres[(i + ri) % P] + offsets[(j + rj) % Q]

so every critical input of that conversion (ties, hi + 1, a double wrap, ...) stands at every row-in-run and lane position of every
tile by construction, and expectation() is the oracle's scalar conversion (qoracle_convert, pinned to the reference's tables by
tests/test_oracle_golden.py) of the P x Q distinct sums, tiled with numpy.  No rounding arithmetic lives here.

K is split into three segments and a zero remainder:
  1. B constant g = eb.raw_max, A the greedy digits of centre // g (sign carried by the digits);
  2. B constant 1, A the digits of centre % g;
  3. A constant 1, B the digits of the offset.
Unsigned operands reach only non-negative targets; build() asserts reachability, the K it needs, and A.B == s in exact integer
arithmetic on the P x Q distinct row / column pairs before it returns anything.  build_stacked() does the same for a complex A whose
parts carry two centre lists against a B that is real or has a zero imaginary part (the stacked plans: C_re = A_re . B_re,
C_im = A_im . B_re)."""
from collections import namedtuple
from math import gcd

import numpy as np

from qublas_amd.desc import SAT, WRP

Designed = namedtuple("Designed", "A B sums centres offsets ri rj k_needed")
# the tile extents and run lengths of the kernels: P and Q are odd, coprime and divide none of them
TILE_EXTENTS = (4, 16, 32, 64, 96, 128, 256)


def digits(target, lo, hi):
    """greedy digits within [lo, hi] that sum to target"""
    out = []
    while target:
        t = min(target, hi) if target > 0 else max(target, lo)
        assert t, "target %d unreachable with digits in [%d, %d]" % (target, lo, hi)
        out.append(t)
        target -= t
    return out


def _split(c, g):
    s = -1 if c < 0 else 1
    q, r = divmod(abs(c), g)
    return s * q, s * r


def segments(ea, eb, centres, offsets):
    """(n1, n2, n3): the lengths of the three segments; their sum is the K the construction needs"""
    g = eb.raw_max
    assert g >= 1 and ea.raw_max >= 1, "the constants 1 and g need a positive operand value"
    n1 = max(len(digits(_split(c, g)[0], ea.raw_min, ea.raw_max)) for c in centres)
    n2 = max(len(digits(_split(c, g)[1], ea.raw_min, ea.raw_max)) for c in centres)
    n3 = max(len(digits(o, eb.raw_min, eb.raw_max)) for o in offsets)
    return n1, n2, n3


def k_needed(ea, eb, centres, offsets):
    return sum(segments(ea, eb, centres, offsets))


def well_formed(P, Q):
    return P % 2 == 1 and Q % 2 == 1 and gcd(P, Q) == 1 and all(t % P and t % Q for t in TILE_EXTENTS)


def build(oracle, ea, eb, es, M, N, K, centres, offsets, ri=0, rj=0, transposed_a=False):
    """host-layout A ([k][i], or [i][k] under TransposedA) and B ([j][k]) of real element types ea, eb with the exact raw dot product
    s(i, j) above in es's unit (es: the last add_args level, which holds every sum); Designed.sums is the P x Q table of s"""
    need = k_needed(ea, eb, centres, offsets)
    assert need <= K, "the construction needs K >= %d, got %d" % (need, K)
    return _build_on(oracle, ea, eb, es, M, N, K, centres, offsets, segments(ea, eb, centres, offsets), ri, rj, transposed_a)


def build_stacked(oracle, ea, eb, es, M, N, K, centres_re, centres_im, offsets, ri=0, rj=0, transposed_a=False):
    """the stacked plans (complex x complex, complex x real): A is complex and its parts carry two independent centre lists of one
    length; B is real, or complex with a zero imaginary part, and carries the shared constants and the offset segment.  Then
    C_re = A_re . B_re and C_im = A_im . B_re exactly, each with its own prescribed sums.  Returns (A, B, Designed of the real parts,
    Designed of the imaginary parts); ea, es: Qcomplex, eb: Qu or Qcomplex"""
    br = eb.real if hasattr(eb, "real") else eb
    P, Q = len(centres_re), len(offsets)
    assert len(centres_im) == P
    need = [segments(part, br, cs, offsets) for part, cs in ((ea.real, centres_re), (ea.imag, centres_im))]
    n1, n2, n3 = (max(a, b) for a, b in zip(*need))
    assert n1 + n2 + n3 <= K, "the construction needs K >= %d, got %d" % (n1 + n2 + n3, K)
    # one real design per part on the common segment lengths: pad the shorter list's segments by building both at the same K with the
    # same constants in B (the segment boundaries are taken from the longer one)
    parts = []
    for part, sp, cs in ((ea.real, es.real, centres_re), (ea.imag, es.imag, centres_im)):
        parts.append(_build_on(oracle, part, br, sp, M, N, K, cs, offsets, (n1, n2, n3), ri, rj, transposed_a))
    assert np.array_equal(parts[0].B, parts[1].B)
    A = np.zeros(M * K, dtype=oracle.host_dtype(ea))
    A["re"], A["im"] = parts[0].A, parts[1].A
    if hasattr(eb, "real"):
        B = np.zeros(K * N, dtype=oracle.host_dtype(eb))
        B["re"] = parts[0].B
    else:
        B = parts[0].B
    return A, B, parts[0], parts[1]


def _build_on(oracle, ea, eb, es, M, N, K, centres, offsets, seg, ri, rj, transposed_a):
    """build() on given segment lengths (at least those the lists need)"""
    centres, offsets = [int(c) for c in centres], [int(o) for o in offsets]
    P, Q = len(centres), len(offsets)
    assert well_formed(P, Q), (P, Q)
    assert es.fracBits == ea.fracBits + eb.fracBits, "the sum format counts in units of the raw product"
    assert ea.isSigned or min(centres) >= 0, "an unsigned A reaches no negative centre"
    assert eb.isSigned or min(offsets) >= 0, "an unsigned B reaches no negative offset"
    g = eb.raw_max
    n1, n2, n3 = seg
    own = segments(ea, eb, centres, offsets)
    assert all(a >= b for a, b in zip(seg, own)) and n1 + n2 + n3 <= K
    need = n1 + n2 + n3
    rows = np.zeros((P, K), dtype=np.int64)
    cols = np.zeros((Q, K), dtype=np.int64)
    cols[:, :n1] = g
    cols[:, n1:n1 + n2] = 1
    rows[:, n1 + n2:need] = 1
    for p, c in enumerate(centres):
        q, r = _split(c, g)
        dq, dr = digits(q, ea.raw_min, ea.raw_max), digits(r, ea.raw_min, ea.raw_max)
        rows[p, :len(dq)] = dq
        rows[p, n1:n1 + len(dr)] = dr
    for p, o in enumerate(offsets):
        do = digits(o, eb.raw_min, eb.raw_max)
        cols[p, n1 + n2:n1 + n2 + len(do)] = do
    assert rows.min() >= ea.raw_min and rows.max() <= ea.raw_max and cols.min() >= eb.raw_min and cols.max() <= eb.raw_max
    sums = [[c + o for o in offsets] for c in centres]
    # the proof, in exact integer arithmetic (int64 where no product sum can leave it, Python integers otherwise): every distinct
    # row x column pair
    if K * max(abs(ea.raw_min), ea.raw_max) * max(abs(eb.raw_min), eb.raw_max) < 1 << 62:
        dots = (rows @ cols.T).tolist()
    else:
        dots = [[sum(int(a) * int(b) for a, b in zip(rows[p, :need], cols[q, :need])) for q in range(Q)] for p in range(P)]
    for p in range(P):
        for q in range(Q):
            assert dots[p][q] == sums[p][q], (p, q, dots[p][q], sums[p][q])
            assert es.raw_min <= sums[p][q] <= es.raw_max, "the sum format does not hold %d" % sums[p][q]
    a = rows[(np.arange(M) + ri) % P]
    b = cols[(np.arange(N) + rj) % Q]
    A = np.ascontiguousarray(a if transposed_a else a.T).reshape(-1).astype(oracle.host_dtype(ea))
    B = np.ascontiguousarray(b).reshape(-1).astype(oracle.host_dtype(eb))
    return Designed(A, B, np.array(sums, dtype=object), centres, offsets, ri, rj, need)


def class_index(dz, M, N):
    """(centre class [N][M], offset class [N][M]) of every element of host-layout C"""
    P, Q = len(dz.centres), len(dz.offsets)
    return np.broadcast_to((np.arange(M) + dz.ri) % P, (N, M)), np.broadcast_to(((np.arange(N) + dz.rj) % Q)[:, None], (N, M))


def converted(oracle, dz, es, ec):
    """the oracle's conversion of the P x Q distinct sums: int64 [P][Q]"""
    return np.array([[oracle.convert_w(int(s), es, ec) for s in row] for row in dz.sums], dtype=np.int64)


def expectation(oracle, dz, es, ec, M, N):
    """host-layout C ([j][i], flat) the designed operands must give"""
    tab = converted(oracle, dz, es, ec)
    pi, qi = class_index(dz, M, N)
    return np.ascontiguousarray(tab[pi, qi]).reshape(-1).astype(oracle.host_dtype(ec))


def geometry(es, ec):
    """(d, unit, H, L, span) in es's unit system: d = F_sum - F_c; for d >= 1 centres count in C's unit = 2^d sum units, and H, L, span
    are C's hi, lo and wrap period; for d <= 0 (no shift, or a left shift) centres count in sum units and H, L are the largest and the
    smallest sum that C holds"""
    d = es.fracBits - ec.fracBits
    W = ec.W
    if d >= 1:
        return d, 1 << d, ec.raw_max, ec.raw_min, (1 << (W + 1)) if ec.isSigned else (1 << W)
    assert W + d >= 2, "C holds fewer than four sums"
    H = (1 << (W + d)) - 1
    return d, 1, H, (-(H + 1) if ec.isSigned else 0), (1 << (W + 1 + d)) if ec.isSigned else (1 << (W + d))


def default_offsets(es, ec, signed=True):
    d, unit, _, _, _ = geometry(es, ec)
    half = unit >> 1
    mags = [1, half, half - 1, half + 1, unit - 1] if d >= 1 else [1, 2]
    out = [0]
    for m in mags:
        for v in ((m, -m) if signed else (m,)):
            if m > 0 and v not in out:
                out.append(v)
    extra = unit + 1 if d >= 1 else 3
    while len(out) % 2 == 0 or len(out) in (1, 3):   # pad to an odd count above 3 with further values
        for v in ((extra, -extra) if signed else (extra,)):
            if v not in out and (len(out) % 2 == 0 or len(out) in (1, 3)):
                out.append(v)
        extra += 1
    return out


def default_centres(es, ec, Q, signed=True, extra=(), reach=None):
    """the critical centres of C's format in sum units, padded to an odd count coprime to Q: around zero, at both bounds, -hi (SAT::SMGN's
    lower bound), and three far outside on each side, of which the last lies beyond two wrap periods.  `reach`: the largest |centre| the
    caller's K allows (a roomy C, whose bounds no short K reaches): centres beyond it are replaced by a spread up to it"""
    d, unit, H, L, span = geometry(es, ec)
    units = [0, 1, -1, 2, -2, 3, -3, H - 1, H, H + 1, L + 1, L, L - 1, -H,
             H + span // 2 + 3, H + span + 2, H + 2 * span + 5, L - span // 2 - 3, L - span - 2, L - 2 * span - 5]
    if reach is not None:
        top = reach // unit
        units = [u for u in units if abs(u) <= top] + [top, -top, top // 2 + 1, -(top // 2) - 1, top // 3, -(top // 3) - 1, top // 5, -(top // 7)]
    out = []
    for u in units:
        c = u * unit
        if (signed or c >= 0) and c not in out:
            out.append(c)
    for c in extra:
        if c not in out:
            out.append(int(c))
    pad = 4
    while not well_formed(len(out), Q):
        for c in ((pad * unit, -pad * unit) if signed else (pad * unit,)):
            if c not in out and not well_formed(len(out), Q):
                out.append(c)
        pad += 1
    return out


def witnesses(oracle, dz, es, ec, signed=True, bounds=True):
    """{name: bool}: the classes of critical conversion inputs that occur among the designed sums (conditions on the data alone).
    Classes that cannot exist for the case (ties without a right shift, the lower side of unsigned sums; with bounds=False, a roomy C:
    everything at C's bounds) are left out."""
    L = oracle.lib()
    d, unit, H, Lo, span = geometry(es, ec)
    flat = [int(s) for row in dz.sums for s in row]
    w = {}
    if d >= 1:
        half, mask = unit >> 1, unit - 1
        kept = lambda s: s >> d
        tie = [s for s in flat if (s & mask) == half]
        w["tie+even"] = any(s > 0 and kept(s) % 2 == 0 for s in tie)
        w["tie+odd"] = any(s > 0 and kept(s) % 2 == 1 for s in tie)
        if d >= 2:
            w["above_half+"] = any(s > 0 and (s & mask) == half + 1 for s in flat)
            w["below_half+"] = any(s > 0 and (s & mask) == half - 1 for s in flat)
        if signed:
            w["tie-even"] = any(s < 0 and kept(s) % 2 == 0 for s in tie)
            w["tie-odd"] = any(s < 0 and kept(s) % 2 == 1 for s in tie)
            if d >= 2:
                w["above_half-"] = any(s < 0 and (s & mask) == half + 1 for s in flat)
                w["below_half-"] = any(s < 0 and (s & mask) == half - 1 for s in flat)
        if not bounds:
            return w
        # the value after rounding, before overflow: the oracle's own rounding primitive
        rounded = [L.qoracle_round(s, d, ec.QuMode) for s in flat]
    elif not bounds:
        return w
    else:
        rounded = flat   # (in sum units: H and Lo are the bounds there)
    want = {"hi": H, "hi+1": H + 1}
    if signed:
        want.update({"lo": Lo, "lo-1": Lo - 1})
        if ec.OfMode == SAT.SMGN and ec.isSigned:
            want.update({"-hi": -H, "-hi-1": -H - 1})
        if not ec.isSigned:
            want.update({"zero": 0, "minus_one": -1})
    for k, v in want.items():
        w[k] = v in rounded
    if ec.OfMode == WRP.TCPL:
        w["multi_wrap+"] = any(r > H + span for r in rounded)
        if signed:
            w["multi_wrap-"] = any(r < Lo - span for r in rounded)
    return w


def shares(oracle, dz, es, ec, M, N, rows=None, cols=None):
    """(in range, above hi, below the lower bound) as fractions of the elements of C[rows, cols] (default: all), by the value after
    rounding"""
    L = oracle.lib()
    d, unit, H, Lo, _ = geometry(es, ec)
    low = -H if (ec.OfMode == SAT.SMGN and ec.isSigned) else Lo
    r = np.array([[L.qoracle_round(int(s), d, ec.QuMode) if d >= 1 else int(s) for s in row] for row in dz.sums], dtype=object)
    cls = np.where(r > H, 1, np.where(r < low, 2, 0)).astype(np.int64)
    # how often each row class and each column class occurs in the block, then the classes' weights
    P, Q = cls.shape
    r0, r1 = rows or (0, M)
    c0, c1 = cols or (0, N)
    wp = np.bincount((np.arange(r0, r1) + dz.ri) % P, minlength=P)
    wq = np.bincount((np.arange(c0, c1) + dz.rj) % Q, minlength=Q)
    w = np.outer(wp, wq)
    return tuple(float(w[cls == k].sum()) / float(w.sum()) for k in range(3))


def table(centres, offsets, ri=0, rj=0):
    """the designed sums alone (no operands): what the witnesses and shares are conditions on"""
    centres, offsets = [int(c) for c in centres], [int(o) for o in offsets]
    return Designed(None, None, np.array([[c + o for o in offsets] for c in centres], dtype=object), centres, offsets, ri, rj, None)


def report(dz, got, exp, M, N, tile):
    """what differs, by (centre, offset) class and tile-local position: the text of a failing comparison"""
    bad = np.flatnonzero(got != exp)
    if not len(bad):
        return ""
    j, i = bad // M, bad % M
    P, Q = len(dz.centres), len(dz.offsets)
    p, q = (i + dz.ri) % P, (j + dz.rj) % Q
    classes = sorted({(dz.centres[a], dz.offsets[b]) for a, b in zip(p[:4096], q[:4096])})
    lines = ["%d of %d elements differ; %d (centre, offset) classes among the first 4096, e.g. %s" % (len(bad), M * N, len(classes), classes[:8]),
             "tile-local rows (mod %d): %s" % (tile, sorted(set((i % tile).tolist()))[:32]),
             "tile-local columns (mod %d): %s" % (tile, sorted(set((j % tile).tolist()))[:32]),
             "tiles (row, column): %s" % sorted(set(zip((i // tile).tolist(), (j // tile).tolist())))[:16]]
    for b in bad[:6]:
        lines.append("  C[i=%d, j=%d]: sum %d -> got %d, expected %d" % (b % M, b // M, dz.sums[(b % M + dz.ri) % P][(b // M + dz.rj) % Q], got[b], exp[b]))
    return "\n".join(lines)
