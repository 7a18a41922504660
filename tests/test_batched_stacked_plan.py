"""The planner of the STACKED batched Qgemul on the CPU (QG_OPT_BATCHED_STACKED: a batch of complex or real x complex members of the
linear class as one block-diagonal launch plus one combine pass; qgemul_classify_batched, qgemul_classify_batched_launches: pure host
code).  Two launches under the flag (six for three members without it: that assertion fails on a library without the feature); the
flag-less answers unchanged — reason, packed bytes, the mixed refusal; the stack's packed bytes; everything the flag must not touch;
the tile-count refusal; the planner under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program
(tests/san/batched_stacked_san_driver.cpp) against the loaded library and a restatement of the geometry; and the two walks of the form
(tests/san/stack_walk_driver.cpp): every tile the GEMM launch writes is read by exactly one part of exactly one output tile."""
import os
import random
import struct
import subprocess

import pytest

from qublas_amd import capi
from qublas_amd.desc import BasicComplexMul, Qcomplex, Qu, RealComplexMul, Tags, TFComplexMul, lower, qgemul_epilogue
from stacked_cases import C5, COMPLEX, LINEAR, UNEQUAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qublas_amd", "csrc")
F = capi.OPT_BATCHED_STACKED
STACKED = b"combine pass"   # what only the stacked form's reason says
TAIL_CPLX, TAIL_MIXED = b"one block-diagonal launch + one combine pass", b"block-diagonal launch + combine pass"
SHAPES = [(33, 17, 40), (64, 64, 64), (65, 40, 200), (130, 170, 264), (1, 1, 1)]


def up(x, m):
    return (x + m - 1) // m * m


def container(ec):
    b = (max(1 + f.intBits + f.fracBits for f in (ec.real, ec.imag)) + 7) // 8
    return 1 << max(0, (b - 1).bit_length())


def mixed_members():
    """(name, A element, B element, C element, keywords, limbs of A and B) of every mixed format, both operand orders"""
    out = []
    for tab in (LINEAR, UNEQUAL):
        for key, (er, ez, ec, kw) in sorted(tab.items()):
            lr, lz = (1, int(key[-1])) if tab is UNEQUAL else (int(key[-1]),) * 2
            out += [("ra_" + key, er, ez, ec, kw, [lr, lz]), ("rb_" + key, ez, er, ec, kw, [lz, lr])]
    return out


def stack_bytes(batch, parts, limbs, rows, K):
    """the members' packed operands back to back — [part][row tile][k tile][limb][64][BK] each — and ONE plane-mask trailer"""
    bk = 128 if limbs == [1, 1] else 64
    return [batch * parts[w] * limbs[w] * up(rows[w], 64) * up(K, bk) + (256 if limbs[w] > 1 else 0) for w in (0, 1)]


def test_complex_members_two_launches_under_the_flag_six_without():
    for key, (e, ec, kw) in sorted(COMPLEX.items()):
        limbs = [int(key[-1])] * 2
        for M, N, K in SHAPES:
            d = lower(e, e, ec, M, N, K, **kw)
            plain = capi.classify(d)
            assert capi.KERNEL_NAMES[plain.kernel] == "mfma_cplx" and list(plain.limbs) == limbs
            # without the flag: member by member on the plain plan's own layout, MFMA launch + combine launch each — as before
            st, info = capi.classify_batched_status(d, 3)
            assert st == capi.QG_OK and capi.classify_batched_launches(d, 3) == 6
            assert list(info.packed_bytes) == [3 * up(b, 256) for b in plain.packed_bytes] and bytes(info.reason) == bytes(plain.reason)
            assert STACKED not in bytes(info.reason)
            # under the flag
            for batch in (1, 3, 300):
                st, info = capi.classify_batched_status(d, batch, F)
                assert st == capi.QG_OK and capi.classify_batched_launches(d, batch, F) == 2, (key, M, N, K, info.reason)
                assert bytes(info.reason).rstrip(b"\0") == b"linear class: %d complex members, " % batch + TAIL_CPLX
                assert capi.KERNEL_NAMES[info.kernel] == "mfma_cplx" and list(info.limbs) == limbs
                assert list(info.packed_bytes) == stack_bytes(batch, (2, 2), limbs, (M, N), K) + [batch * up(2 * M * N * container(ec), 256)]
                assert info.ops == batch * plain.ops == batch * 8.0 * M * N * K


def test_mixed_members_served_under_the_flag_refused_without():
    for name, ea, eb, ec, kw, limbs in mixed_members():
        for M, N, K in SHAPES:
            d = lower(ea, eb, ec, M, N, K, **kw)
            plain = capi.classify(d)
            assert capi.KERNEL_NAMES[plain.kernel] == "mfma_rc" and list(plain.limbs) == limbs
            st, info = capi.classify_batched_status(d, 3)
            assert st == capi.QG_EUNSUPPORTED and b"mixed real-complex" in bytes(info.reason) and not info.supported
            assert capi.classify_batched_launches(d, 3) == capi.QG_EUNSUPPORTED
            parts = (1, 2) if name.startswith("ra") else (2, 1)
            form = b"real x complex" if name.startswith("ra") else b"complex x real"
            for batch in (1, 3, 300):
                st, info = capi.classify_batched_status(d, batch, F)
                assert st == capi.QG_OK and capi.classify_batched_launches(d, batch, F) == 2, (name, M, N, K, info.reason)
                assert bytes(info.reason).rstrip(b"\0") == b"linear class: %d %s members, " % (batch, form) + TAIL_MIXED
                assert capi.KERNEL_NAMES[info.kernel] == "mfma_rc" and list(info.limbs) == limbs
                assert list(info.packed_bytes) == stack_bytes(batch, parts, limbs, (M, N), K) + [batch * up(2 * M * N * container(ec), 256)]
                assert info.ops == batch * plain.ops == batch * 4.0 * M * N * K


def same_answer(d, batch=3):
    a, b = capi.classify_batched_status(d, batch), capi.classify_batched_status(d, batch, F)
    assert a[0] == b[0] and bytes(a[1]) == bytes(b[1]), (a[1].reason, b[1].reason)
    assert capi.classify_batched_launches(d, batch) == capi.classify_batched_launches(d, batch, F)
    assert STACKED not in bytes(b[1].reason)
    return a


def test_the_flag_changes_nothing_else():
    e43, e88 = Qu(4, 3), Qu(8, 8)
    e, ec, kw = COMPLEX["limb2"]
    er, ez, ecm, kwm = LINEAR["limb2"]
    # real members: the block-diagonal form, the tree class, a composite plan
    real = lower(e43, e43, Qu(16, 3), 65, 33, 100, mul_args=Tags(9, 6), add_args=[Qu(19, 6)])
    same_answer(real)
    assert capi.classify_batched_launches(real, 3, F) == 1
    same_answer(lower(e88, e88, e88, 33, 17, 40))
    same_answer(lower(e43, e43, Qu(30, 3), 64, 64, 140000, mul_args=Tags(9, 6), add_args=[Qu(27, 6)]), 2)
    # a tree-class complex member
    st, info = same_answer(lower(C5, C5, C5, 33, 17, 40, mul_args=TFComplexMul()))
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] == "tree_cplx_i32"
    # a complex member whose K leaves the one-launch range (2 limbs x K beyond 2^17 - 1): the tree kernels, member by member
    st, info = same_answer(lower(e, e, Qcomplex(Qu(30, 4), Qu(30, 0)), 8, 8, 70000, **kw))
    assert st == capi.QG_OK and capi.KERNEL_NAMES[info.kernel] != "mfma_cplx"
    # a mixed member outside the form is refused exactly as without the flag: the tree class, and K beyond the range
    for d in (lower(e43, C5, Qcomplex(Qu(14, 3), Qu(14, 3)), 33, 17, 40), lower(er, ez, ecm, 8, 8, 70000, **kwm)):
        st, info = same_answer(d)
        assert st == capi.QG_EUNSUPPORTED and b"mixed real-complex: no batched or grouped plan" in bytes(info.reason)
    # a member large enough for the two-group kernels: no block-diagonal variant, member by member
    st, info = same_answer(lower(e, e, ec, 2049, 1921, 200, **kw), 2)
    assert st == capi.QG_OK and capi.classify_batched_launches(lower(e, e, ec, 2049, 1921, 200, **kw), 2, F) == 4
    # plain and grouped plans
    dc, dm = lower(e, e, ec, 65, 40, 200, **kw), lower(er, ez, ecm, 65, 40, 200, **kwm)
    for d in (dc, dm):
        assert bytes(capi.classify(d)) == bytes(capi.classify(d, F))
    for group in ([dc, dc], [dc, dm]):
        a, b = capi.classify_grouped_status(group), capi.classify_grouped_status(group, F)
        assert a[0] == b[0] and bytes(a[1]) == bytes(b[1])
        assert capi.classify_grouped_launches(group) == capi.classify_grouped_launches(group, F)
    assert capi.classify_grouped_status([dc, dm], F)[0] == capi.QG_EUNSUPPORTED
    # the _batched_epx entries: a complex and a mixed member are refused as before
    ep = qgemul_epilogue()
    for d in (dc, dm):
        ep.d = d.c[0]
        a, b = capi.classify_batched_epx_status(d, 3, ep), capi.classify_batched_epx_status(d, 3, ep, flags=F)
        assert a[0] == b[0] != capi.QG_OK and bytes(a[1]) == bytes(b[1])
        assert capi.classify_batched_epx_launches(d, 3, ep) == capi.classify_batched_epx_launches(d, 3, ep, flags=F) < 0


def test_more_than_2_31_tiles_is_einval():
    e, ec, kw = COMPLEX["limb1"]
    one = lower(e, e, ec, 64, 64, 64, **kw)          # 1 x 1 part tiles: four tiles per member in the launch
    assert capi.classify_batched_status(one, 2 ** 29 - 1, F)[0] == capi.QG_OK
    st, info = capi.classify_batched_status(one, 2 ** 29, F)
    assert st == capi.QG_EINVAL and b"2^31 - 1 tiles" in bytes(info.reason) and capi.classify_batched_launches(one, 2 ** 29, F) == capi.QG_EINVAL
    assert capi.classify_batched_status(one, 2 ** 29)[0] == capi.QG_OK   # (member by member: no tile count to overflow)
    er, ez, ecm, kwm = LINEAR["limb1"]
    two = lower(er, ez, ecm, 64, 64, 64, **kwm)      # mixed: two tiles per member
    assert capi.classify_batched_status(two, 2 ** 30 - 1, F)[0] == capi.QG_OK
    assert capi.classify_batched_status(two, 2 ** 30, F)[0] == capi.QG_EINVAL
    six = lower(e, e, ec, 65, 129, 64, **kw)         # 2 x 3 part tiles: 24 tiles per member
    assert capi.classify_batched_status(six, (2 ** 31 - 1) // 24, F)[0] == capi.QG_OK
    assert capi.classify_batched_status(six, (2 ** 31 - 1) // 24 + 1, F)[0] == capi.QG_EINVAL
    for batch in (0, -1):
        assert capi.classify_batched_status(one, batch, F)[0] == capi.QG_EINVAL


# ---- the planner as a stand-alone program under the sanitizers
def random_members(n, seed):
    """complex and mixed descriptors of the linear class (one to three limbs per operand, K inside and beyond the one-launch range),
    tree-class ones (default tags) and a few real ones"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        M, N, K = rng.randint(1, 300), rng.randint(1, 300), rng.choice([1, 7, 40, 200, 264, 3000, 70000])
        lg = max(1, (K - 1).bit_length())
        kind = rng.random()
        ta = rng.random() < 0.3
        if kind < 0.45:      # complex x complex, every sub-product and level exact
            w = rng.choice([6, 12, 17])
            e = Qcomplex(Qu(w - 3, 3), Qu(w - 5, 5))
            p = lambda x, y: Qu(x.intBits + y.intBits + 1, x.fracBits + y.fracBits)
            ac, bd, ad, bc = p(e.real, e.real), p(e.imag, e.imag), p(e.real, e.imag), p(e.imag, e.real)
            re, im = Qu(max(ac.intBits, bd.intBits) + 1, max(ac.fracBits, bd.fracBits)), Qu(ad.intBits + 1, ad.fracBits)
            lv = Qcomplex(Qu(re.intBits + lg, re.fracBits), Qu(im.intBits + lg, im.fracBits))
            out.append(lower(e, e, lv, M, N, K, transposed_a=ta, mul_args=BasicComplexMul(acT=ac, bdT=bd, adT=ad, bcT=bc, acbdT=re, adbcT=im), add_args=[lv]))
        elif kind < 0.85:    # mixed
            wr, wz = rng.choice([6, 12, 17]), rng.choice([6, 12, 17])
            er, ez = Qu(wr - 3, 3), Qcomplex(Qu(wz - 2, 2), Qu(wz - 4, 4))
            pr, pi = Qu(er.intBits + ez.real.intBits + 2, 5), Qu(er.intBits + ez.imag.intBits + 2, 7)
            lv = Qcomplex(Qu(pr.intBits + lg, 5), Qu(pi.intBits + lg, 7))
            ea, eb = (er, ez) if rng.random() < 0.5 else (ez, er)
            out.append(lower(ea, eb, lv, M, N, K, transposed_a=ta, mul_args=RealComplexMul(realT=pr, imagT=pi), add_args=[lv]))
        elif kind < 0.93:    # tree class
            out.append(lower(C5, C5, C5, M, N, min(K, 3000), transposed_a=ta, mul_args=TFComplexMul()) if rng.random() < 0.5 else
                       lower(Qu(4, 3), C5, Qcomplex(Qu(14, 3), Qu(14, 3)), M, N, min(K, 3000), transposed_a=ta))
        else:                # real
            out.append(lower(Qu(8, 8), Qu(8, 8), Qu(24, 8), M, N, min(K, 3000), transposed_a=ta, mul_args=Tags(17, 16), add_args=[Qu(29, 16)]))
    return out


def test_the_batched_planner_under_sanitizers(tmp_path):
    exe = str(tmp_path / "batched_stacked_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "batched_stacked_san_driver.cpp"), os.path.join(CSRC, "qg_geom.cpp"), os.path.join(CSRC, "qg_plan.cpp"), "-o", exe])
    descs = random_members(400, 21)
    batches = [1, 3, 9, 300, 1024, 7, 1 << 29, 1 << 40, 0, 2]
    flag_sets = [F, 0, F | capi.OPT_FORCE_TREE, F, 0, F | capi.OPT_GENERIC_LAYOUT]
    queries = [(flag_sets[i % 6], batches[(i // 6) % len(batches)] if i % 7 else 3, d) for i, d in enumerate(descs)]
    wire = b"".join(struct.pack("<Iq", f, b) + bytes(d) for f, b, d in queries)
    r = subprocess.run([exe], input=wire, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"ERROR" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(queries)
    seen = {}
    for (f, batch, d), line in zip(queries, lines):
        st, i = capi.classify_batched_status(d, batch, f)
        ok = st == capi.QG_OK
        launches = capi.classify_batched_launches(d, batch, f)
        assert (launches > 0) == ok and (ok or launches == st)
        stacked = ok and STACKED in bytes(i.reason)
        # the member block of the launch and its workspace, restated: parts x tile-padded rows over 64, 64 x 64 int64 per tile
        pa, pb = (2 if d.cmul != 3 else 1), (2 if d.cmul != 4 else 1)
        tm, tn = pa * up(d.M, 64) // 64, pb * up(d.N, 64) // 64
        z = lambda v: v if ok else 0
        want = "st=%d sup=%d kernel=%d limbs=%d,%d packed=%d,%d,%d ops=%s launches=%d stack=%d tiles=%d,%d ws=%d reason=%s" % (
            st, i.supported if batch >= 1 else 0, z(i.kernel), z(i.limbs[0]), z(i.limbs[1]), z(i.packed_bytes[0]), z(i.packed_bytes[1]), z(i.packed_bytes[2]),
            "%.17g" % (i.ops if ok else 0.0), z(launches), ((1 if d.cmul not in (3, 4) else d.cmul - 1) if stacked else 0), tm if stacked else 0, tn if stacked else 0,
            batch * tm * tn * 4096 * 8 if stacked else 0, i.reason.decode() if batch >= 1 else "")
        assert line == want, (line, want)
        # (members of at most 300 x 300: every complex or mixed MFMA plan among them has a block-diagonal variant)
        assert stacked == (ok and bool(f & F) and capi.KERNEL_NAMES[i.kernel] in ("mfma_cplx", "mfma_rc")), line
        assert not stacked or launches == 2
        key = (st, "stacked" if stacked else capi.KERNEL_NAMES.get(i.kernel) if ok else None)
        seen[key] = seen.get(key, 0) + 1
    # every answer is exercised: the form, a complex member by member without the flag, the mixed refusal, the tile-count refusal
    for key, least in (((capi.QG_OK, "stacked"), 40), ((capi.QG_OK, "mfma_cplx"), 3), ((capi.QG_EUNSUPPORTED, None), 10), ((capi.QG_EINVAL, None), 10)):
        assert seen.get(key, 0) >= least, (key, seen)


# ---- the two walks of the form: the GEMM launch over the doubled tile counts, the combine pass over one part's
def test_every_workspace_tile_is_written_once_and_read_once(tmp_path):
    exe = str(tmp_path / "stack_walk")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "stack_walk_driver.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    walks = {}
    for ln in r.stdout.decode().splitlines():
        head, _, vals = ln.partition(" :")
        kind, *key = head.split()
        walks[(kind,) + tuple(int(x) for x in key)] = [int(x) for x in vals.split()]
    n = 0
    for mode in (1, 2, 3):
        for tm in (1, 2, 3, 8, 9, 17):
            for tn in (1, 2, 3, 5):
                for batch in (1, 2, 9):
                    bd_tm, bd_tn = tm * (2 if mode in (1, 3) else 1), tn * (2 if mode in (1, 2) else 1)
                    total = batch * bd_tm * bd_tn
                    # the GEMM launch: a bijection of its workgroups onto the workspace's tiles
                    assert sorted(walks[("gemm", mode, tm, tn, batch)]) == list(range(total)), (mode, tm, tn, batch)
                    # the combine pass: a bijection of its workgroups onto (member, output tile), and its source tiles — both parts',
                    # every product's — cover the workspace's tiles exactly once: inside the member's own block, at the quadrants
                    v = walks[("comb", mode, tm, tn, batch)]
                    per = 3 + (4 if mode == 1 else 2)
                    recs = [v[i:i + per] for i in range(0, len(v), per)]
                    assert sorted(tuple(x[:3]) for x in recs) == [(b, m, c) for b in range(batch) for m in range(tm) for c in range(tn)]
                    assert sorted(t for x in recs for t in x[3:]) == list(range(total)), (mode, tm, tn, batch)
                    for b, lm, ln, *src in recs:
                        at = lambda r, c: (b * bd_tm + r) * bd_tn + c
                        if mode == 1:     # re: (lm, ln), (lm + tm, ln + tn); im: (lm, ln + tn), (lm + tm, ln)
                            assert src == [at(lm, ln), at(lm + tm, ln + tn), at(lm, ln + tn), at(lm + tm, ln)]
                        elif mode == 2:   # real x complex: B's parts side by side
                            assert src == [at(lm, ln), at(lm, ln + tn)]
                        else:             # complex x real: A's parts one above the other
                            assert src == [at(lm, ln), at(lm + tm, ln)]
                    n += 1
    assert n == 3 * 6 * 4 * 3
