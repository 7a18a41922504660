"""qublas_amd/csrc/qg_tile_walk.h on the CPU: the swizzle of the packed operands' LDS image, the XCD-aware order of the output
tiles and the persistent kernels' tile lists are plain integer functions, so the host compiler builds them (with
-fsanitize=address,undefined, as tests/test_plan_sanitizers.py builds the planner) and this test compares what they print with
the arithmetic the kernels carried inline before they shared the header, restated here.  Every corner of the walk is met:
tile rows that are no multiple of the group size, tile counts that are no multiple of 8, fewer tiles than workgroups."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENTS = range(1, 41)
GRIDS = (8, 16, 24, 256, 304)


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_walk") / "tile_walk")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           os.path.join(ROOT, "tests", "san", "tile_walk_driver.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr.decode()[-3000:]
    out = {"swz": [], "walk": {}, "list": {}}
    for ln in r.stdout.decode().splitlines():
        kind, _, rest = ln.partition(" ")
        if kind == "swz":
            out["swz"].append(tuple(int(x) for x in rest.split()))
        else:
            key, _, vals = rest.partition(" :")
            out[kind][tuple(int(x) for x in key.split())] = [int(x) for x in vals.split()]
    return out


def run_start(nwg, x):
    """first tile number of XCD residue class x: the run split as the kernels spelled it"""
    q, r = nwg // 8, nwg % 8
    return x * (q + 1) if x < r else r * (q + 1) + (x - r) * q


def tile_of(w, tiles_m, tiles_n, gm):
    """tile number -> (tile_m, tile_n): groups of gm tile rows, column by column"""
    grp = w // (gm * tiles_n)
    first_m = grp * gm
    gsz = min(tiles_m - first_m, gm)
    rem = w % (gm * tiles_n)
    return first_m + rem % gsz, rem // gsz


def test_swizzle(printed):
    assert [s[0] for s in printed["swz"]] == list(range(256))
    for r, s64, s128, r64, r128 in printed["swz"]:
        assert s64 == (0, 2, 3, 1)[(r // 4) % 4], r
        assert s128 == (r // 2) % 8, r
        assert (r64, r128) == (s64, s128), r          # the run-time-bk form of the pack kernels


@pytest.mark.parametrize("gm", [8, 16])
def test_lock_step_walk(printed, gm):
    n = 0
    for tiles_m in EXTENTS:
        for tiles_n in EXTENTS:
            nwg = tiles_m * tiles_n
            exp = []
            for bid in range(nwg):
                tm, tn = tile_of(run_start(nwg, bid % 8) + bid // 8, tiles_m, tiles_n, gm)
                exp.append(tm * 64 + tn)
            assert sorted(exp) == sorted(m * 64 + c for m in range(tiles_m) for c in range(tiles_n))    # (the restatement itself: a bijection)
            for mod in (0, 1):                                                                           # both spellings of the position in the group
                got = printed["walk"][(gm, mod, tiles_m, tiles_n)]
                assert got == exp, (gm, mod, tiles_m, tiles_n)
                n += 1
    assert n == 2 * len(EXTENTS) ** 2


def test_persistent_lists(printed):
    n = 0
    for tiles_m in EXTENTS:
        for tiles_n in EXTENTS:
            nwg = tiles_m * tiles_n
            for grid in GRIDS:
                v = printed["list"][(tiles_m, tiles_n, grid)]
                assert len(v) == 3 * grid
                seen = bytearray(nwg)
                total = 0
                P = grid // 8
                for b in range(grid):
                    first, step, count = v[3 * b:3 * b + 3]
                    x, j = b % 8, b // 8
                    start, cnt = run_start(nwg, x), nwg // 8 + (1 if x < nwg % 8 else 0)
                    # the restatement
                    assert (first, step, count) == (start + j, P, (cnt - j + P - 1) // P if j < cnt else 0), (tiles_m, tiles_n, grid, b)
                    if j >= cnt:
                        assert count == 0             # a workgroup beyond its class's tiles has nothing to do
                        continue
                    # the list stays inside the run of its residue class
                    assert start <= first and first + step * (count - 1) < start + cnt, (tiles_m, tiles_n, grid, b)
                    seen[first:first + step * count:step] = b"\x01" * count
                    total += count
                # every tile number exactly once: as many list entries as tiles, and none left out
                assert total == nwg and seen.count(1) == nwg, (tiles_m, tiles_n, grid)
                assert sum(1 for b in range(grid) if v[3 * b + 2]) <= nwg
                n += 1
    assert n == len(EXTENTS) ** 2 * len(GRIDS)
