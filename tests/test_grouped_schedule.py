"""The host-side schedule of a grouped launch (qublas_amd/csrc/qg_grp.h) on the CPU: the host compiler builds the header with
-fsanitize=address,undefined (as tests/test_tile_walk_batched.py does) and this test compares every record it prints, for swept
groups, with a restatement.

The restated rule.  DEALT order: members sorted by decreasing k-tile count, ties by list index; each member's tiles in the order
qg_tile_of<8, true> walks them; that sequence is cut into chunks of 8 tiles and chunk c goes to the residue class c % 8 of the block
id, inside a class in sequence order — for the first 64 * (T // 64) tiles, i.e. whole rounds of 8 chunks, which fill the block ids
below 64 * (T // 64) exactly.  LEFTOVER: the tail of the sequence (fewer than 64 tiles, the shortest k-loops) takes the remaining
block ids in sequence order.  MEMBER order: tile number w of the list-order sequence goes to the block id b with qg_xcd_block(b, T) == w."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A_BLK, B_BLK, C_TILE = 2 * 64 * 64, 3 * 64 * 64, 64 * 64
TILES = {(1, 1), (2, 1), (3, 3), (9, 2), (17, 5)}
NKS = {1, 2, 3, 8, 1024}


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grouped_schedule") / "grouped_schedule")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "grouped_schedule_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    return [json.loads(l) for l in r.stdout.decode().splitlines()]


def tile_of(w, tiles_m, tiles_n, gm=8):
    """qg_tile_of<8, true>"""
    grp = w // (gm * tiles_n)
    first = grp * gm
    gsz = min(tiles_m - first, gm)
    rem = w % (gm * tiles_n)
    return first + rem % gsz, rem // gsz


def xcd_block(bid, nwg):
    q, r, x = nwg // 8, nwg % 8, bid % 8
    return (x * (q + 1) if x < r else r * (q + 1) + (x - r) * q) + bid // 8


def prefix(members):
    """where every member starts: the prefix sums of the members' block sizes"""
    out, a, b, c, ra, rb = [], 0, 0, 0, 0, 0
    for tm, tn, nk in members:
        out.append((a, b, c, ra, rb))
        a += tm * nk * A_BLK
        b += tn * nk * B_BLK
        c += tm * tn * C_TILE
        ra += tm * 64
        rb += tn * 64
    return out


def record(members, starts, g, w):
    tm, tn, nk = members[g]
    a, b, c, ra, rb = starts[g]
    lm, ln = tile_of(w, tm, tn)
    return [a + lm * nk * A_BLK, b + ln * nk * B_BLK, c + (lm * tn + ln) * C_TILE, g * 1000003 - 17, nk, ra + lm * 64, rb + ln * 64, g]


def restated(members, mode):
    starts = prefix(members)
    order = sorted(range(len(members)), key=lambda g: (-members[g][2], g)) if mode == 0 else list(range(len(members)))
    seq = [record(members, starts, g, w) for g in order for w in range(members[g][0] * members[g][1])]
    T = len(seq)
    table = [None] * T
    if mode == 0:
        dealt = T // 64 * 64
        for s, rec in enumerate(seq):
            chunk, e = divmod(s, 8)
            table[chunk % 8 + 8 * (chunk // 8 * 8 + e) if s < dealt else s] = rec
    else:
        for b in range(T):
            table[b] = seq[xcd_block(b, T)]
    return table


def test_the_sweep_covers_the_sizes_and_every_option(printed):
    assert sorted({len(p["members"]) for p in printed}) == [1, 2, 7, 8, 9, 300]
    assert {p["mode"] for p in printed} == {0, 1}
    assert {(m[0], m[1]) for p in printed for m in p["members"]} == TILES
    assert {m[2] for p in printed for m in p["members"]} == NKS
    assert any(len(p["table"]) % 64 for p in printed) and any(len(p["table"]) > 64 * 8 for p in printed)


def test_record_for_record_equal_to_the_restatement(printed):
    for p in printed:
        assert p["table"] == restated([tuple(m) for m in p["members"]], p["mode"]), (p["mode"], len(p["members"]))


def test_bijection_onto_the_tiles_and_offsets_are_prefix_sums(printed):
    for p in printed:
        members = [tuple(m) for m in p["members"]]
        starts = prefix(members)
        want = sorted(tuple(record(members, starts, g, w)) for g in range(len(members)) for w in range(members[g][0] * members[g][1]))
        assert sorted(tuple(r) for r in p["table"]) == want
        assert len({(r[7], r[2]) for r in p["table"]}) == len(p["table"]) == sum(m[0] * m[1] for m in members)
        for r in p["table"]:
            a, b, c, ra, rb = starts[r[7]]
            tm, tn, nk = members[r[7]]
            assert r[4] == nk and r[0] % 1024 == 0 and r[1] % 1024 == 0
            assert a <= r[0] < a + tm * nk * A_BLK and b <= r[1] < b + tn * nk * B_BLK and c <= r[2] < c + tm * tn * C_TILE
            assert ra <= r[5] < ra + tm * 64 and rb <= r[6] < rb + tn * 64


def test_dealt_order_never_lets_nk_increase_along_a_residue_class(printed):
    for p in printed:
        if p["mode"] != 0:
            continue
        nk = [r[4] for r in p["table"]]
        for x in range(8):
            cls = nk[x::8]
            assert all(cls[i] >= cls[i + 1] for i in range(len(cls) - 1)), (x, len(p["members"]))


def test_the_eight_tiles_of_a_dealt_chunk_sit_in_one_class(printed):
    for p in printed:
        if p["mode"] != 0:
            continue
        members = [tuple(m) for m in p["members"]]
        starts = prefix(members)
        order = sorted(range(len(members)), key=lambda g: (-members[g][2], g))
        seq = [tuple(record(members, starts, g, w)) for g in order for w in range(members[g][0] * members[g][1])]
        where = {tuple(r): b for b, r in enumerate(p["table"])}
        for c in range(len(seq) // 64 * 8):
            assert len({where[r] % 8 for r in seq[8 * c:8 * c + 8]}) == 1, c
